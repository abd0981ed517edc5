// cc_replay_eval.h — host side of the frame scatter of a replayed sequence: per stream and for the caller's columns (cc_engine_scatter_info /
// _apply), and for all streams per call with the label compare behind it, the replay evaluator (cc_replay_eval_*). ABI: include/cc_kitti.h;
// kernels: cc_k_replay_eval.h, where both paths share scatter_column_info / scatter_column_apply; DESIGN.md sections 9 and 18.
// Not a header of its own: cc_engine.hip includes it once, at its end, behind everything it calls (cc_engine, CC_HIP_CHECK, stop_resident,
// finish_batch, ensure_gather). The evaluator's handle owns all of its memory from create to destroy; a step enqueues on the engine's stream and counts its own kernel
// launches and synchronisations.

struct cc_replay_eval
{
    cc_engine* e{nullptr};
    int S{0}, slots{0}, lanes{0}, R{0}, NC{0}, ring_cols{0};
    int64_t max_points{0};
    unsigned table{0};
    // device
    int32_t* d_org{nullptr};
    uint16_t* d_sem{nullptr};
    uint32_t* d_eu{nullptr};
    uint8_t* d_ground{nullptr};
    uint32_t* d_det{nullptr};
    long long* d_npts{nullptr};
    cck::ReplayState* d_state{nullptr};
    cc_replay_stream* d_plan{nullptr};
    cck::ReplayWalk* d_walk{nullptr};
    cck::ReplayJob* d_jobs{nullptr};
    cck::ReplayCtl* d_ctl{nullptr};
    int *d_min{nullptr}, *d_max{nullptr}; // [S][ring_cols]
    unsigned long long *d_keys{nullptr}, *d_counts{nullptr}, *d_npairs{nullptr};
    unsigned* d_vals{nullptr};
    std::vector<void*> device_blocks;
    // pinned host
    cc_replay_stream* h_plan{nullptr};
    cck::ReplayCtl* h_ctl{nullptr};
    cck::ReplayJob* h_jobs{nullptr};
    unsigned char* h_finish{nullptr};
    unsigned long long *h_counts{nullptr}, *h_npairs{nullptr};
    cck::ReplayPair* h_pairs{nullptr};
    size_t pair_capacity{0};
    std::vector<void*> pinned_blocks;
    // staging of add_frame: a ring of blocks {n_points, semantic, euclid}, an event behind each block's last copy
    std::vector<unsigned char*> h_stage;
    std::vector<hipEvent_t> stage_ev;
    std::vector<char> stage_used;
    size_t stage_next{0}, stage_sem_off{0}, stage_eu_off{0};
    // host mirrors (exact: every change goes through this handle)
    std::vector<int> prev, active;
    std::vector<long long> npts; // [S][slots]
    int job_capacity{0};
    uint64_t steps{0}, launches{0}, syncs{0}, rounds{0};
};

namespace
{

template<class T>
int replay_device(cc_replay_eval* h, T** out, size_t count)
{
    void* p = nullptr;
    const hipError_t err = hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
    if (err != hipSuccess)
    {
        h->e->error = std::string("cc_replay_eval_create: hipMalloc: ") + hipGetErrorString(err);
        return CC_ERR_HIP;
    }
    h->device_blocks.push_back(p);
    *out = (T*) p;
    return CC_OK;
}

template<class T>
int replay_pinned(cc_replay_eval* h, T** out, size_t count)
{
    void* p = nullptr;
    const hipError_t err = hipHostMalloc(&p, std::max<size_t>(count, 1) * sizeof(T));
    if (err != hipSuccess)
    {
        h->e->error = std::string("cc_replay_eval_create: hipHostMalloc: ") + hipGetErrorString(err);
        return CC_ERR_HIP;
    }
    h->pinned_blocks.push_back(p);
    *out = (T*) p;
    return CC_OK;
}

void replay_free(cc_replay_eval* h)
{
    for (hipEvent_t ev : h->stage_ev)
        (void) hipEventDestroy(ev);
    for (void* p : h->device_blocks)
        (void) hipFree(p);
    for (void* p : h->pinned_blocks)
        (void) hipHostFree(p);
    delete h;
}

int replay_slot_of(const cc_replay_eval* h, int64_t frame)
{
    const int64_t m = frame % h->slots;
    return (int) (m < 0 ? m + h->slots : m);
}

// the shape the handle was created for is still the engine's
int replay_check_shape(cc_replay_eval* h, const char* who)
{
    const cc_engine* e = h->e;
    if (e->g.num_streams != h->S || e->g.num_rows != h->R || e->g.num_columns != h->NC || e->g.ring_cols != h->ring_cols)
    {
        h->e->error = std::string(who) + ": the engine's shape changed since cc_replay_eval_create";
        return CC_ERR_INVALID_ARGUMENT;
    }
    return CC_OK;
}

// the rounds of the label compare over jobs [0, n) of d_jobs / h_jobs: records[i] of job i. Two launches and one synchronisation per round.
int replay_evaluate(cc_replay_eval* h, int64_t n, cc_replay_record* records)
{
    cc_engine* e = h->e;
    hipStream_t q = e->stream;
    std::vector<std::vector<ccev::Pair>> pairs((size_t) h->lanes);
    for (int64_t first = 0; first < n; first += h->lanes)
    {
        const int in_round = (int) std::min<int64_t>(h->lanes, n - first);
        long long most = 0;
        for (int l = 0; l < in_round; l++)
        {
            const cck::ReplayJob j = h->h_jobs[first + l];
            most = std::max(most, h->npts[(size_t) j.stream * h->slots + replay_slot_of(h, j.frame)]);
        }
        const unsigned blocks = (unsigned) std::max<long long>((most + 255) / 256, 1);
        hipLaunchKernelGGL(cck::k_replay_eval, dim3(blocks, (unsigned) in_round), dim3(256), 0, q, (const cck::ReplayJob*) h->d_jobs, (int) first, h->slots,
                           (long long) h->max_points, (const long long*) h->d_npts, (const uint16_t*) h->d_sem, (const uint32_t*) h->d_eu,
                           (const unsigned char*) h->d_ground, (const unsigned*) h->d_det, h->d_counts, h->d_keys, h->d_vals, h->table, h->d_npairs);
        hipLaunchKernelGGL(cck::k_replay_compact, dim3((h->table + 255) / 256, (unsigned) in_round), dim3(256), 0, q, h->table, h->d_keys, h->d_vals, h->d_counts,
                           h->d_npairs, (unsigned long long) h->pair_capacity, h->h_pairs, h->h_counts);
        h->launches += 2;
        CC_HIP_CHECK(e, hipGetLastError());
        CC_HIP_CHECK(e, hipMemcpyAsync(h->h_npairs, h->d_npairs, 8, hipMemcpyDeviceToHost, q));
        CC_HIP_CHECK(e, hipStreamSynchronize(q));
        h->syncs++;
        h->rounds++;
        const unsigned long long np = *h->h_npairs;
        if (np > h->pair_capacity)
        {
            e->error = "cc_replay_eval: more distinct label pairs than points";
            return CC_ERR_BOOKKEEPING;
        }
        for (int l = 0; l < in_round; l++)
            pairs[(size_t) l].clear();
        for (unsigned long long i = 0; i < np; i++)
        {
            const cck::ReplayPair& p = h->h_pairs[i];
            if (p.lane < (unsigned) in_round)
                pairs[p.lane].push_back(ccev::Pair{(uint32_t) (p.key >> 32), (uint32_t) p.key, p.count});
        }
        for (int l = 0; l < in_round; l++)
        {
            const unsigned long long* c = h->h_counts + (size_t) l * cck::REPLAY_COUNTS;
            cc_replay_record& rec = records[first + l];
            memset(&rec, 0, sizeof(rec));
            rec.stream = h->h_jobs[first + l].stream;
            rec.frame = h->h_jobs[first + l].frame;
            rec.r.tp = (double) c[0];
            rec.r.fn = (double) c[1];
            rec.r.fp = (double) c[2];
            rec.r.tn = (double) c[3];
            if (c[4])
                pairs[(size_t) l].push_back(ccev::Pair{0xffffffffu, 0xffffffffu, (unsigned) c[4]});
            ccev::sum_entropies(pairs[(size_t) l], &rec.r);
        }
    }
    return CC_OK;
}

// what every entry point that enqueues on the engine's stream does first
int replay_enter(cc_replay_eval* h, const char* who, bool finish)
{
    cc_engine* e = h->e;
    (void) hipSetDevice(e->device);
    int rc = stop_resident(e);
    if (rc)
        return rc;
    if (finish && (rc = finish_batch(e)))
        return rc;
    return replay_check_shape(h, who);
}

} // namespace

extern "C" {

// ---- frame scatter of a replayed sequence (kitti_demo.cpp:173-224), include/cc_kitti.h ------------------------------------------------
int cc_engine_scatter_info(cc_engine* e, int n, const int32_t* streams, const int64_t* from, const int64_t* to, const int32_t* d_original_index,
                           int slots, int32_t* h_min_frame, int32_t* h_max_frame)
{
    if (!e || n < 0 || slots < 1 || (n > 0 && (!streams || !from || !to || !d_original_index || !h_min_frame || !h_max_frame)))
        return CC_ERR_INVALID_ARGUMENT;
    (void) hipSetDevice(e->device);
    int rc = stop_resident(e);
    if (rc)
        return rc;
    rc = finish_batch(e);
    if (rc)
        return rc;
    size_t total = 0;
    for (int i = 0; i < n; i++)
    {
        if (streams[i] < 0 || streams[i] >= e->g.num_streams || from[i] < 0 || to[i] - from[i] >= e->g.ring_cols)
            return CC_ERR_INVALID_ARGUMENT; // (columns outside the stream's published ring window read as empty: the kernels check)
        if (to[i] >= from[i])
            total += (size_t) (to[i] - from[i] + 1);
    }
    if (total == 0)
        return CC_OK;
    if ((rc = ensure_gather(e, total * 8 + 64)))
        return rc;
    int* d_min = (int*) e->d_gather;
    int* d_max = d_min + total;
    size_t o = 0;
    for (int i = 0; i < n; i++)
        if (to[i] >= from[i])
        {
            const unsigned cols = (unsigned) (to[i] - from[i] + 1);
            hipLaunchKernelGGL(cck::k_scatter_info, dim3(cols), dim3(64), 0, e->stream, e->g, e->P, (const StreamState*) e->d_states, streams[i], (long long) from[i], d_original_index,
                               slots, d_min + o, d_max + o);
            o += cols;
        }
    CC_HIP_CHECK(e, hipGetLastError());
    CC_HIP_CHECK(e, hipMemcpyAsync(h_min_frame, d_min, total * 4, hipMemcpyDeviceToHost, e->stream));
    CC_HIP_CHECK(e, hipMemcpyAsync(h_max_frame, d_max, total * 4, hipMemcpyDeviceToHost, e->stream));
    CC_HIP_CHECK(e, hipStreamSynchronize(e->stream));
    return CC_OK;
}

int cc_engine_scatter_apply(cc_engine* e, int stream, int64_t from, int64_t to, const int32_t* d_original_index, int slots, uint8_t* d_is_ground,
                            uint32_t* d_detection, int64_t max_points)
{
    if (!e || stream < 0 || stream >= e->g.num_streams || slots < 1 || !d_original_index || !d_is_ground || !d_detection || max_points < 1 ||
        from < 0 || to - from >= e->g.ring_cols)
        return CC_ERR_INVALID_ARGUMENT;
    if (to < from)
        return CC_OK;
    (void) hipSetDevice(e->device);
    int rc = stop_resident(e);
    if (rc)
        return rc;
    rc = finish_batch(e);
    if (rc)
        return rc;
    hipLaunchKernelGGL(cck::k_scatter_apply, dim3((unsigned) (to - from + 1)), dim3(64), 0, e->stream, e->g, e->P, (const StreamState*) e->d_states, stream, (long long) from,
                       d_original_index, slots, d_is_ground, d_detection, (long long) max_points);
    CC_HIP_CHECK(e, hipGetLastError());
    return CC_OK; // (asynchronous on cc_engine_hip_stream(e): cc_eval_frame_device on the same stream, or cc_engine_sync, orders behind it)
}

int cc_replay_eval_create(cc_replay_eval** out, cc_engine* e, int slots, int64_t max_points, int eval_lanes)
{
    if (!out || !e)
        return CC_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (slots < 1 || slots > 1024 || max_points < 1 || max_points > (1ll << 30) || eval_lanes < 1 || eval_lanes > 65535)
    {
        e->error = "cc_replay_eval_create: slots must be 1..1024, max_points 1..2^30, eval_lanes 1..65535";
        return CC_ERR_INVALID_ARGUMENT;
    }
    (void) hipSetDevice(e->device);
    int rc = stop_resident(e);
    if (rc)
        return rc;
    if ((rc = finish_batch(e)))
        return rc;
    cc_replay_eval* h = new cc_replay_eval();
    h->e = e;
    h->S = e->g.num_streams;
    h->R = e->g.num_rows;
    h->NC = e->g.num_columns;
    h->ring_cols = e->g.ring_cols;
    h->slots = slots;
    h->lanes = eval_lanes;
    h->max_points = max_points;
    h->table = ccev::table_size(max_points);
    h->job_capacity = h->S * (slots + 1);
    const size_t S = (size_t) h->S, SL = S * (size_t) slots, MP = (size_t) max_points, L = (size_t) eval_lanes;
    const size_t org_n = SL * (size_t) h->NC * (size_t) h->R;
    h->pair_capacity = L * MP;
    const size_t sem_bytes = (MP * 2 + 15) / 16 * 16;
    h->stage_sem_off = 16;
    h->stage_eu_off = 16 + sem_bytes;
    const size_t stage_bytes = 16 + sem_bytes + MP * 4;
    if ((rc = replay_device(h, &h->d_org, org_n)) || (rc = replay_device(h, &h->d_sem, SL * MP)) || (rc = replay_device(h, &h->d_eu, SL * MP)) ||
        (rc = replay_device(h, &h->d_ground, SL * MP)) || (rc = replay_device(h, &h->d_det, SL * MP)) || (rc = replay_device(h, &h->d_npts, SL)) ||
        (rc = replay_device(h, &h->d_state, S)) || (rc = replay_device(h, &h->d_plan, S)) || (rc = replay_device(h, &h->d_walk, S)) ||
        (rc = replay_device(h, &h->d_jobs, (size_t) h->job_capacity)) || (rc = replay_device(h, &h->d_ctl, 1)) ||
        (rc = replay_device(h, &h->d_min, S * (size_t) h->ring_cols)) || (rc = replay_device(h, &h->d_max, S * (size_t) h->ring_cols)) ||
        (rc = replay_device(h, &h->d_keys, L * h->table)) || (rc = replay_device(h, &h->d_vals, L * h->table)) ||
        (rc = replay_device(h, &h->d_counts, L * cck::REPLAY_COUNTS)) || (rc = replay_device(h, &h->d_npairs, 1)) ||
        (rc = replay_pinned(h, &h->h_plan, S)) || (rc = replay_pinned(h, &h->h_ctl, 1)) || (rc = replay_pinned(h, &h->h_jobs, (size_t) h->job_capacity)) ||
        (rc = replay_pinned(h, &h->h_finish, S)) || (rc = replay_pinned(h, &h->h_counts, L * cck::REPLAY_COUNTS)) ||
        (rc = replay_pinned(h, &h->h_npairs, 1)) || (rc = replay_pinned(h, &h->h_pairs, h->pair_capacity)))
    {
        replay_free(h);
        return rc;
    }
    for (size_t i = 0; i < S; i++)
    {
        unsigned char* p = nullptr;
        hipEvent_t ev = nullptr;
        if ((rc = replay_pinned(h, &p, stage_bytes)))
        {
            replay_free(h);
            return rc;
        }
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess)
        {
            e->error = "cc_replay_eval_create: hipEventCreate failed";
            replay_free(h);
            return CC_ERR_HIP;
        }
        h->h_stage.push_back(p);
        h->stage_ev.push_back(ev);
        h->stage_used.push_back(0);
    }
    h->prev.assign(S, 0);
    h->active.assign(S, 1);
    h->npts.assign(SL, 0);
    std::vector<cck::ReplayState> init(S);
    for (auto& st : init)
    {
        st.cursor = 0;
        st.error_column = -1;
        st.prev = 0;
        st.active = 1;
        st.error = 0;
        st.pad = 0;
    }
    hipStream_t q = e->stream;
    // (in stream order and waited for: recycled device memory is not zero, and `init` leaves scope)
    if (hipMemsetAsync(h->d_org, 0xFF, org_n * 4, q) != hipSuccess || hipMemsetAsync(h->d_sem, 0, SL * MP * 2, q) != hipSuccess ||
        hipMemsetAsync(h->d_eu, 0, SL * MP * 4, q) != hipSuccess || hipMemsetAsync(h->d_ground, 0, SL * MP, q) != hipSuccess ||
        hipMemsetAsync(h->d_det, 0, SL * MP * 4, q) != hipSuccess || hipMemsetAsync(h->d_npts, 0, SL * 8, q) != hipSuccess ||
        hipMemsetAsync(h->d_keys, 0xFF, L * h->table * 8, q) != hipSuccess || hipMemsetAsync(h->d_vals, 0, L * h->table * 4, q) != hipSuccess ||
        hipMemsetAsync(h->d_counts, 0, L * cck::REPLAY_COUNTS * 8, q) != hipSuccess || hipMemsetAsync(h->d_npairs, 0, 8, q) != hipSuccess ||
        hipMemcpyAsync(h->d_state, init.data(), S * sizeof(cck::ReplayState), hipMemcpyHostToDevice, q) != hipSuccess ||
        hipStreamSynchronize(q) != hipSuccess)
    {
        e->error = "cc_replay_eval_create: initialising the device blocks failed";
        replay_free(h);
        return CC_ERR_HIP;
    }
    memset(h->h_finish, 0, S);
    *out = h;
    return CC_OK;
}

void cc_replay_eval_destroy(cc_replay_eval* h)
{
    if (!h)
        return;
    (void) hipSetDevice(h->e->device);
    (void) stop_resident(h->e);
    (void) hipStreamSynchronize(h->e->stream); // (copies and kernels of this handle may still be in flight)
    replay_free(h);
}

int32_t* cc_replay_eval_original_index(cc_replay_eval* h, int stream, int64_t frame)
{
    if (!h || stream < 0 || stream >= h->S)
        return nullptr;
    return h->d_org + ((size_t) stream * (size_t) h->slots + (size_t) replay_slot_of(h, frame)) * (size_t) h->NC * (size_t) h->R;
}

int cc_replay_eval_slot_arrays(cc_replay_eval* h, int stream, int64_t frame, uint8_t** d_is_ground, uint32_t** d_detection)
{
    if (!h || stream < 0 || stream >= h->S)
        return CC_ERR_INVALID_ARGUMENT;
    const size_t o = ((size_t) stream * (size_t) h->slots + (size_t) replay_slot_of(h, frame)) * (size_t) h->max_points;
    if (d_is_ground)
        *d_is_ground = h->d_ground + o;
    if (d_detection)
        *d_detection = h->d_det + o;
    return CC_OK;
}

int cc_replay_eval_add_frame(cc_replay_eval* h, int stream, int64_t frame, int64_t n_points, const uint16_t* semantic, const uint32_t* euclid)
{
    if (!h)
        return CC_ERR_INVALID_ARGUMENT;
    cc_engine* e = h->e;
    const char* bad = nullptr;
    if (stream < 0 || stream >= h->S)
        bad = "no such stream";
    else if (frame < 0 || frame > 0x7fffffff)
        bad = "frame must be 0 .. 2^31 - 1";
    else if (n_points < 0 || n_points > h->max_points)
        bad = "n_points exceeds max_points";
    else if (n_points > 0 && (!semantic || !euclid))
        bad = "semantic and euclid must not be NULL";
    else if (frame >= (int64_t) h->prev[(size_t) stream] + h->slots)
        bad = "frame >= previous_frame + slots: its slot still belongs to a frame that has not been evaluated";
    if (bad)
    {
        e->error = std::string("cc_replay_eval_add_frame: ") + bad;
        return CC_ERR_INVALID_ARGUMENT;
    }
    int rc = replay_enter(h, "cc_replay_eval_add_frame", false);
    if (rc)
        return rc;
    hipStream_t q = e->stream;
    const size_t k = h->stage_next;
    h->stage_next = (k + 1) % h->h_stage.size();
    if (h->stage_used[k])
        CC_HIP_CHECK(e, hipEventSynchronize(h->stage_ev[k])); // (only when every block of the ring is in flight: no step since S frames)
    unsigned char* st = h->h_stage[k];
    const long long n = (long long) n_points;
    memcpy(st, &n, 8);
    if (n > 0)
    {
        memcpy(st + h->stage_sem_off, semantic, (size_t) n * 2);
        memcpy(st + h->stage_eu_off, euclid, (size_t) n * 4);
    }
    const size_t fs = (size_t) stream * (size_t) h->slots + (size_t) replay_slot_of(h, frame);
    const size_t o = fs * (size_t) h->max_points, MP = (size_t) h->max_points;
    CC_HIP_CHECK(e, hipMemcpyAsync(h->d_npts + fs, st, 8, hipMemcpyHostToDevice, q));
    if (n > 0)
    {
        CC_HIP_CHECK(e, hipMemcpyAsync(h->d_sem + o, st + h->stage_sem_off, (size_t) n * 2, hipMemcpyHostToDevice, q));
        CC_HIP_CHECK(e, hipMemcpyAsync(h->d_eu + o, st + h->stage_eu_off, (size_t) n * 4, hipMemcpyHostToDevice, q));
    }
    CC_HIP_CHECK(e, hipMemsetAsync(h->d_ground + o, 0, MP, q));
    CC_HIP_CHECK(e, hipMemsetAsync(h->d_det + o, 0, MP * 4, q));
    CC_HIP_CHECK(e, hipEventRecord(h->stage_ev[k], q));
    h->stage_used[k] = 1;
    h->npts[fs] = n;
    return CC_OK;
}

int cc_replay_eval_set_active(cc_replay_eval* h, int stream, int active)
{
    if (!h || stream < 0 || stream >= h->S)
        return CC_ERR_INVALID_ARGUMENT;
    int rc = replay_enter(h, "cc_replay_eval_set_active", false);
    if (rc)
        return rc;
    hipLaunchKernelGGL(cck::k_replay_poke, dim3(1), dim3(1), 0, h->e->stream, h->d_state, stream, 0, 0ll, 0, 1, active ? 1 : 0);
    CC_HIP_CHECK(h->e, hipGetLastError());
    h->active[(size_t) stream] = active ? 1 : 0;
    return CC_OK;
}

int cc_replay_eval_seek(cc_replay_eval* h, int stream, int64_t column, int32_t previous_frame)
{
    if (!h || stream < 0 || stream >= h->S || column < 0)
        return CC_ERR_INVALID_ARGUMENT;
    int rc = replay_enter(h, "cc_replay_eval_seek", false);
    if (rc)
        return rc;
    hipLaunchKernelGGL(cck::k_replay_poke, dim3(1), dim3(1), 0, h->e->stream, h->d_state, stream, 1, (long long) column, (int) previous_frame, 0, 0);
    CC_HIP_CHECK(h->e, hipGetLastError());
    h->prev[(size_t) stream] = previous_frame;
    return CC_OK;
}

int cc_replay_eval_step(cc_replay_eval* h, const uint8_t* finish, cc_replay_record* records, int64_t capacity, int64_t* n_records, cc_replay_stream* h_table)
{
    if (!h)
        return CC_ERR_INVALID_ARGUMENT;
    cc_engine* e = h->e;
    if (capacity < 0 || (!records && capacity != 0) || !n_records || !h_table)
    {
        e->error = "cc_replay_eval_step: capacity must be >= 0 (0 without a record array), n_records and h_table must not be NULL";
        return CC_ERR_INVALID_ARGUMENT;
    }
    if (e->resident_opt)
    {
        e->error = "cc_replay_eval_step: not available while the option \"resident\" is on (the resident kernel owns the stream's state); set it to 0 first";
        return CC_ERR_INVALID_ARGUMENT;
    }
    int rc = replay_enter(h, "cc_replay_eval_step", true);
    if (rc)
        return rc;
    const int S = h->S;
    hipStream_t q = e->stream;
    h->steps++;
    for (int s = 0; s < S; s++)
        h->h_finish[s] = finish ? (finish[s] != 0 ? 1 : 0) : 0;
    hipLaunchKernelGGL(cck::k_replay_plan, dim3((unsigned) ((S + 63) / 64)), dim3(64), 0, q, e->g, (const StreamState*) e->d_states,
                       (const cck::ReplayState*) h->d_state, h->d_plan, h->h_plan);
    h->launches++;
    CC_HIP_CHECK(e, hipGetLastError());
    CC_HIP_CHECK(e, hipStreamSynchronize(q));
    h->syncs++;
    // the grids follow the longest range of the plan, not the ring
    int64_t longest = 0;
    for (int s = 0; s < S; s++)
        longest = std::max<int64_t>(longest, h->h_plan[s].col_to - h->h_plan[s].col_from);
    if (longest > h->ring_cols)
    {
        e->error = "cc_replay_eval_step: a range longer than the ring";
        return CC_ERR_BOOKKEEPING;
    }
    const int stride = (int) std::max<int64_t>(longest, 1);
    if (longest > 0)
    {
        hipLaunchKernelGGL(cck::k_replay_info, dim3((unsigned) longest, (unsigned) S), dim3(64), 0, q, e->g, e->P, (const cc_replay_stream*) h->d_plan,
                           (const int*) h->d_org, h->slots, h->d_min, h->d_max, stride);
        h->launches++;
    }
    hipLaunchKernelGGL(cck::k_replay_walk, dim3((unsigned) S), dim3(64), 0, q, (const cc_replay_stream*) h->d_plan, (const cck::ReplayState*) h->d_state,
                       (const int*) h->d_min, (const int*) h->d_max, stride, h->slots, (const unsigned char*) h->h_finish, h->d_walk);
    hipLaunchKernelGGL(cck::k_replay_scan, dim3(1), dim3(cck::TAKE_SCAN_THREADS), 0, q, S, h->d_plan, (const cck::ReplayWalk*) h->d_walk, h->d_state,
                       (long long) capacity, h->job_capacity, h->d_jobs, h->h_jobs, h->d_ctl, h->h_plan, h->h_ctl);
    h->launches += 2;
    if (longest > 0) // (the kernel looks at the verdict itself: nothing is applied unless every record fits)
    {
        hipLaunchKernelGGL(cck::k_replay_apply, dim3((unsigned) longest, (unsigned) S), dim3(64), 0, q, e->g, e->P, (const cc_replay_stream*) h->d_plan,
                           (const cck::ReplayCtl*) h->d_ctl, (const int*) h->d_org, h->slots, h->d_ground, h->d_det, (long long) h->max_points);
        h->launches++;
    }
    CC_HIP_CHECK(e, hipGetLastError());
    CC_HIP_CHECK(e, hipStreamSynchronize(q));
    h->syncs++;
    memcpy(h_table, h->h_plan, (size_t) S * sizeof(cc_replay_stream));
    const int64_t total = h->h_ctl->total;
    *n_records = total;
    if (!h->h_ctl->fits)
    {
        e->error = "cc_replay_eval_step: " + std::to_string(total) + " records do not fit a capacity of " + std::to_string(capacity) +
                   " (nothing was applied or evaluated, no cursor moved)";
        return CC_ERR_CAPACITY;
    }
    for (int s = 0; s < S; s++)
    {
        h->prev[(size_t) s] = h->h_plan[s].previous_frame;
        h->active[(size_t) s] = h->h_plan[s].active;
    }
    return replay_evaluate(h, total, records);
}

int cc_replay_eval_evaluate_slots(cc_replay_eval* h, int stream, int n, const int32_t* frames, cc_replay_record* records)
{
    if (!h || stream < 0 || stream >= h->S || n < 0 || n > h->job_capacity || (n > 0 && (!frames || !records)))
        return CC_ERR_INVALID_ARGUMENT;
    int rc = replay_enter(h, "cc_replay_eval_evaluate_slots", true);
    if (rc)
        return rc;
    if (n == 0)
        return CC_OK;
    for (int i = 0; i < n; i++)
    {
        h->h_jobs[i].stream = stream;
        h->h_jobs[i].frame = frames[i];
    }
    CC_HIP_CHECK(h->e, hipMemcpyAsync(h->d_jobs, h->h_jobs, (size_t) n * sizeof(cck::ReplayJob), hipMemcpyHostToDevice, h->e->stream));
    return replay_evaluate(h, n, records);
}

int cc_replay_eval_counters(cc_replay_eval* h, uint64_t* steps, uint64_t* kernel_launches, uint64_t* host_syncs, uint64_t* eval_rounds)
{
    if (!h)
        return CC_ERR_INVALID_ARGUMENT;
    if (steps)
        *steps = h->steps;
    if (kernel_launches)
        *kernel_launches = h->launches;
    if (host_syncs)
        *host_syncs = h->syncs;
    if (eval_rounds)
        *eval_rounds = h->rounds;
    return CC_OK;
}

} // extern "C"
