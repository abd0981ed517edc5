// cc_take.h — host side of the hand-overs in device memory: cc_engine_take_points / _take_cursor / _take_seek (kernels: cc_k_take.h, DESIGN.md
// section 15) and cc_engine_take_clusters / _take_clusters_cursor (cc_k_take_clusters.h, section 16). Not a header of its own: cc_engine.hip
// includes it once, at its end, behind everything it calls (cc_engine, CC_HIP_CHECK, alloc_plane, alloc_pinned, grow_scratch, query_stream,
// finish_batch). The lower end a cursor query reports is cck::held_from (cc_k_held.h), the one the plan kernels start from.

namespace
{

struct TakeBlock // a device block of a take: the engine's member that names it, its size
{
    void** member;
    size_t bytes;
};

// The pinned mirror and the device blocks of a take, by its first call (the device blocks again after a change of shape: free_all). blocks[0] is
// the cursor array: it starts at zero, and it is what says that the blocks exist. The members are set once every block is there: a call that
// fails half way leaves nothing behind that a later call would take for complete.
int ensure_take_blocks(cc_engine* e, char** pinned, size_t pinned_bytes, const TakeBlock* blocks, int n)
{
    int rc;
    if (!*pinned && (rc = alloc_pinned(e, pinned, pinned_bytes, PIN_ENGINE)))
        return rc;
    if (*blocks[0].member)
        return CC_OK;
    std::vector<char*> got((size_t) n, nullptr);
    for (int i = 0; i < n; i++)
        if ((rc = alloc_plane(e, &got[(size_t) i], blocks[i].bytes)))
            return rc;
    // (in stream order and waited for: a hipMemset on the null stream is not ordered against the engine's streams, and recycled device memory is not zero)
    CC_HIP_CHECK(e, hipMemsetAsync(got[0], 0, blocks[0].bytes, query_stream(e)));
    CC_HIP_CHECK(e, hipStreamSynchronize(query_stream(e)));
    for (int i = n - 1; i >= 0; i--)
        *blocks[i].member = got[(size_t) i];
    return CC_OK;
}

// cc_engine_take_points: the cursors [2 stages][streams], the plan, the control block
int ensure_take(cc_engine* e)
{
    const size_t S = (size_t) e->g.num_streams;
    const TakeBlock blocks[] = {{(void**) &e->d_take_cursor, 2 * S * sizeof(long long)},
                                {(void**) &e->d_take_plan, S * sizeof(cc_take_stream)},
                                {(void**) &e->d_take_ctl, sizeof(cck::TakeCtl)}};
    return ensure_take_blocks(e, &e->h_take, S * sizeof(cc_take_stream) + sizeof(cck::TakeCtl), blocks, 3);
}

// cc_engine_take_clusters: the cursor pairs, the plan, the table, the control block
int ensure_take_clusters(cc_engine* e)
{
    const size_t S = (size_t) e->g.num_streams;
    const TakeBlock blocks[] = {{(void**) &e->d_tc_cursor, 2 * S * sizeof(long long)},
                                {(void**) &e->d_tc_plan, S * sizeof(cck::TcPlan)},
                                {(void**) &e->d_tc_table, S * sizeof(cc_take_cluster_stream)},
                                {(void**) &e->d_tc_ctl, sizeof(cck::TcCtl)}};
    return ensure_take_blocks(e, &e->h_tc, S * (sizeof(cck::TcPlan) + sizeof(cc_take_cluster_stream)) + sizeof(cck::TcCtl), blocks, 4);
}

// what the take functions share: arguments, the resident kernel, the batches in flight, the buffers
int take_enter(cc_engine* e, const char* who, int stage)
{
    if (!e)
        return CC_ERR_INVALID_ARGUMENT;
    if (stage != CC_TAKE_CLUSTERED && stage != CC_TAKE_SEGMENTED)
    {
        e->error = std::string(who) + ": stage must be CC_TAKE_CLUSTERED or CC_TAKE_SEGMENTED";
        return CC_ERR_INVALID_ARGUMENT;
    }
    if (e->resident_opt)
    {
        e->error = std::string(who) + ": not available while the option \"resident\" is on (the resident kernel owns the stream's state); set it to 0 first";
        return CC_ERR_INVALID_ARGUMENT;
    }
    (void) hipSetDevice(e->device);
    int rc = finish_batch(e);
    if (rc)
        return rc;
    return ensure_take(e);
}

} // namespace

extern "C" {

// ---- hand-over of the published points (cc_k_take.h) ----------------------------------------------------------------
int cc_engine_take_points(cc_engine* e, int stage, int select, cc_take_point* d_records, int64_t capacity, cc_take_stream* d_table,
                          cc_take_stream* h_table, int64_t* n_records)
{
    if (!e)
        return CC_ERR_INVALID_ARGUMENT;
    const char* bad = nullptr;
    if (select != CC_TAKE_ALL_RETURNS && select != CC_TAKE_NOT_GROUND && select != CC_TAKE_WITH_ID)
        bad = "select must be CC_TAKE_ALL_RETURNS, CC_TAKE_NOT_GROUND or CC_TAKE_WITH_ID";
    else if (select == CC_TAKE_WITH_ID && stage == CC_TAKE_SEGMENTED)
        bad = "CC_TAKE_WITH_ID needs the CLUSTERED stage (segmented columns have no final ids)";
    else if (capacity < 0 || (!d_records && capacity != 0))
        bad = "capacity must be >= 0, and 0 without a record array (the size query)";
    else if (((uintptr_t) d_records & 15u) != 0)
        bad = "d_records must be 16-byte aligned";
    else if (!h_table || !n_records)
        bad = "h_table and n_records must not be NULL";
    if (bad)
    {
        e->error = std::string("cc_engine_take_points: ") + bad;
        return CC_ERR_INVALID_ARGUMENT;
    }
    int rc = take_enter(e, "cc_engine_take_points", stage);
    if (rc)
        return rc;
    const int S = e->g.num_streams;
    hipStream_t q = query_stream(e);
    cc_take_stream* h_plan = (cc_take_stream*) e->h_take;
    cck::TakeCtl* h_ctl = (cck::TakeCtl*) (e->h_take + (size_t) S * sizeof(cc_take_stream));
    hipLaunchKernelGGL(cck::k_take_plan, dim3((unsigned) ((S + 63) / 64)), dim3(64), 0, q, e->g, e->d_states, e->d_take_cursor, stage, e->d_take_plan, h_plan);
    CC_HIP_CHECK(e, hipGetLastError());
    CC_HIP_CHECK(e, hipStreamSynchronize(q));
    // the grids follow the longest range of the plan, not the ring
    int64_t longest = 0;
    for (int s = 0; s < S; s++)
        longest = std::max<int64_t>(longest, h_plan[s].col_to - h_plan[s].col_from);
    if (longest > e->g.ring_cols)
    {
        e->error = "cc_engine_take_points: a range longer than the ring";
        return CC_ERR_BOOKKEEPING;
    }
    const int stride = (int) std::max<int64_t>(longest, 1);
    // (twice what is needed, at most a ring per stream: ranges that creep up from take to take must not allocate a new block each time)
    const size_t counts_need = (size_t) S * (size_t) stride;
    if ((rc = grow_scratch(e, &e->d_take_counts, &e->take_counts_cap, counts_need, std::min(2 * counts_need, (size_t) S * (size_t) e->g.ring_cols))))
        return rc;
    if (longest > 0)
        hipLaunchKernelGGL(cck::k_take_count, dim3((unsigned) longest, (unsigned) S), dim3(64), 0, q, e->g, e->P, e->d_take_plan, select, e->d_take_counts, stride);
    hipLaunchKernelGGL(cck::k_take_scan, dim3((unsigned) S), dim3(cck::TAKE_SCAN_THREADS), 0, q, e->d_take_plan, e->d_take_counts, stride);
    hipLaunchKernelGGL(cck::k_take_scan_streams, dim3(1), dim3(cck::TAKE_SCAN_THREADS), 0, q, S, e->d_take_plan, (long long) capacity, d_records ? 1 : 0,
                       e->d_take_ctl, d_table, h_plan, h_ctl);
    if (d_records) // (the kernel looks at the verdict itself: nothing is written and no cursor moves unless every record fits)
        hipLaunchKernelGGL(cck::k_take_write, dim3((unsigned) stride, (unsigned) S), dim3(64), 0, q, e->g, e->P, e->d_take_plan, e->d_take_ctl, stage, select,
                           e->d_take_counts, stride, d_records, e->d_take_cursor);
    CC_HIP_CHECK(e, hipGetLastError());
    CC_HIP_CHECK(e, hipStreamSynchronize(q));
    memcpy(h_table, h_plan, (size_t) S * sizeof(cc_take_stream));
    *n_records = h_ctl->total;
    if (h_ctl->total > capacity)
    {
        e->error = "cc_engine_take_points: " + std::to_string(h_ctl->total) + " records do not fit a capacity of " + std::to_string(capacity) +
                   " (nothing was written, no cursor moved)";
        return CC_ERR_CAPACITY;
    }
    return CC_OK;
}

int cc_engine_take_cursor(cc_engine* e, int stage, int stream, int64_t* cursor, int64_t* readable_from)
{
    if (!e || stream < 0 || stream >= e->g.num_streams)
        return CC_ERR_INVALID_ARGUMENT;
    int rc = take_enter(e, "cc_engine_take_cursor", stage);
    if (rc)
        return rc;
    long long cur = 0;
    StreamState st;
    CC_HIP_CHECK(e, hipMemcpy(&cur, e->d_take_cursor + (size_t) stage * e->g.num_streams + stream, sizeof(cur), hipMemcpyDeviceToHost));
    CC_HIP_CHECK(e, hipMemcpy(&st, e->d_states + stream, sizeof(st), hipMemcpyDeviceToHost));
    if (cursor)
        *cursor = cur;
    if (readable_from)
        *readable_from = cck::held_from(st.first_column, st.clear_done, 0);
    return CC_OK;
}

int cc_engine_take_seek(cc_engine* e, int stage, int stream, int64_t column)
{
    if (!e || stream < -1 || stream >= e->g.num_streams || column < 0)
        return CC_ERR_INVALID_ARGUMENT;
    int rc = take_enter(e, "cc_engine_take_seek", stage);
    if (rc)
        return rc;
    const int first = stream < 0 ? 0 : stream, count = stream < 0 ? e->g.num_streams : 1;
    const std::vector<long long> v((size_t) count, (long long) column);
    CC_HIP_CHECK(e, hipMemcpy(e->d_take_cursor + (size_t) stage * e->g.num_streams + first, v.data(), (size_t) count * sizeof(long long), hipMemcpyHostToDevice));
    return CC_OK;
}

// ---- hand-over of the finished clusters (cc_k_take_clusters.h) ------------------------------------------------------
int cc_engine_take_clusters(cc_engine* e, uint32_t min_points, int flags, cc_take_cluster* d_clusters, int64_t cluster_capacity, cc_take_point* d_records,
                            int64_t record_capacity, cc_take_cluster_stream* d_table, cc_take_cluster_stream* h_table, int64_t* n_clusters,
                            int64_t* n_records)
{
    if (!e)
        return CC_ERR_INVALID_ARGUMENT;
    const bool with_points = flags == CC_TAKE_CLUSTERS_WITH_POINTS;
    const char* bad = nullptr;
    if (flags != CC_TAKE_CLUSTERS_WITH_POINTS && flags != CC_TAKE_CLUSTERS_DESCRIPTORS_ONLY)
        bad = "flags must be CC_TAKE_CLUSTERS_WITH_POINTS or CC_TAKE_CLUSTERS_DESCRIPTORS_ONLY";
    else if (cluster_capacity < 0 || (!d_clusters && cluster_capacity != 0))
        bad = "cluster_capacity must be >= 0, and 0 without a descriptor array (the size query)";
    else if (record_capacity < 0 || (!d_records && record_capacity != 0))
        bad = "record_capacity must be >= 0, and 0 without a record array";
    else if (d_clusters && with_points && !d_records)
        bad = "d_records must not be NULL unless CC_TAKE_CLUSTERS_DESCRIPTORS_ONLY is set";
    else if (((uintptr_t) d_clusters & 15u) != 0 || ((uintptr_t) d_records & 15u) != 0)
        bad = "d_clusters and d_records must be 16-byte aligned";
    else if (((uintptr_t) d_table & 7u) != 0)
        bad = "d_table must be 8-byte aligned";
    else if (!h_table || !n_clusters || !n_records)
        bad = "h_table, n_clusters and n_records must not be NULL";
    if (bad)
    {
        e->error = std::string("cc_engine_take_clusters: ") + bad;
        return CC_ERR_INVALID_ARGUMENT;
    }
    int rc = take_enter(e, "cc_engine_take_clusters", CC_TAKE_CLUSTERED);
    if (rc || (rc = ensure_take_clusters(e)))
        return rc;
    const int S = e->g.num_streams;
    hipStream_t q = query_stream(e);
    cck::TcPlan* h_plan = (cck::TcPlan*) e->h_tc;
    cc_take_cluster_stream* h_tab = (cc_take_cluster_stream*) (e->h_tc + (size_t) S * sizeof(cck::TcPlan));
    cck::TcCtl* h_ctl = (cck::TcCtl*) (e->h_tc + (size_t) S * (sizeof(cck::TcPlan) + sizeof(cc_take_cluster_stream)));
    hipLaunchKernelGGL(cck::k_tc_plan, dim3(1), dim3(cck::TAKE_SCAN_THREADS), 0, q, e->g, e->d_states, e->d_tc_cursor, e->d_tc_plan, e->d_tc_table, h_plan, h_ctl);
    CC_HIP_CHECK(e, hipGetLastError());
    CC_HIP_CHECK(e, hipStreamSynchronize(q));
    // the grids follow the plan: the longest column range, the longest id range, the ids of all streams
    int64_t longest_cols = 0, longest_ids = 0;
    for (int s = 0; s < S; s++)
    {
        longest_cols = std::max<int64_t>(longest_cols, h_plan[s].col_to - h_plan[s].col_from);
        longest_ids = std::max<int64_t>(longest_ids, h_plan[s].n_ids);
    }
    const int64_t total_ids = h_ctl->total_ids;
    if (longest_cols > e->g.ring_cols || total_ids < 0 || total_ids + S > 0x7fffffffll)
    {
        e->error = "cc_engine_take_clusters: a range longer than the ring, or more ids than a grid has blocks";
        return CC_ERR_BOOKKEEPING;
    }
    // (twice what is needed: id counts that creep up from take to take must not allocate a new block each time)
    const size_t slots_need = (size_t) std::max<int64_t>(total_ids, 1);
    if ((rc = grow_scratch(e, &e->d_tc_slots, &e->tc_slots_cap, slots_need, 2 * slots_need)))
        return rc;
    if (total_ids > 0)
    {
        hipLaunchKernelGGL(cck::k_tc_clear, dim3((unsigned) ((longest_ids + cck::TAKE_SCAN_THREADS - 1) / cck::TAKE_SCAN_THREADS), (unsigned) S),
                           dim3(cck::TAKE_SCAN_THREADS), 0, q, e->d_tc_plan, e->d_tc_slots, (long long) total_ids);
        if (longest_cols > 0)
            hipLaunchKernelGGL(cck::k_tc_mark, dim3((unsigned) longest_cols, (unsigned) S), dim3(64), 0, q, e->g, e->P, e->d_tc_plan, e->d_tc_table,
                               e->d_tc_slots, (long long) total_ids);
    }
    hipLaunchKernelGGL(cck::k_tc_scan, dim3((unsigned) S), dim3(cck::TAKE_SCAN_THREADS), 0, q, e->d_tc_plan, e->d_tc_table, e->d_tc_slots, (long long) total_ids,
                       (unsigned) min_points);
    hipLaunchKernelGGL(cck::k_tc_scan_streams, dim3(1), dim3(cck::TAKE_SCAN_THREADS), 0, q, S, e->d_tc_table, (long long) cluster_capacity,
                       (long long) record_capacity, d_clusters ? 1 : 0, with_points ? 1 : 0, (long long) total_ids, e->d_tc_ctl, d_table, h_tab, h_ctl);
    if (d_clusters) // (the kernel looks at the verdict itself: nothing is written and no cursor moves unless everything fits)
        hipLaunchKernelGGL(cck::k_tc_write, dim3((unsigned) (S + total_ids)), dim3(64), 0, q, e->g, e->P, e->d_tc_plan, e->d_tc_table, e->d_tc_ctl, e->d_tc_slots,
                           (long long) total_ids, d_clusters, with_points ? d_records : nullptr, e->d_tc_cursor);
    CC_HIP_CHECK(e, hipGetLastError());
    CC_HIP_CHECK(e, hipStreamSynchronize(q));
    memcpy(h_table, h_tab, (size_t) S * sizeof(cc_take_cluster_stream));
    *n_clusters = h_ctl->clusters;
    *n_records = h_ctl->records;
    if (h_ctl->clusters > cluster_capacity || (with_points && h_ctl->records > record_capacity))
    {
        e->error = "cc_engine_take_clusters: " + std::to_string(h_ctl->clusters) + " clusters with " + std::to_string(h_ctl->records) +
                   " records do not fit capacities of " + std::to_string(cluster_capacity) + " and " + std::to_string(record_capacity) +
                   " (nothing was written, no cursor moved)";
        return CC_ERR_CAPACITY;
    }
    return CC_OK;
}

int cc_engine_take_clusters_cursor(cc_engine* e, int stream, int64_t* next_id, int64_t* floor_column, int64_t* readable_from)
{
    if (!e || stream < 0 || stream >= e->g.num_streams)
        return CC_ERR_INVALID_ARGUMENT;
    int rc = take_enter(e, "cc_engine_take_clusters_cursor", CC_TAKE_CLUSTERED);
    if (rc || (rc = ensure_take_clusters(e)))
        return rc;
    long long cur[2] = {0, 0};
    StreamState st;
    CC_HIP_CHECK(e, hipMemcpy(cur, e->d_tc_cursor + 2 * (size_t) stream, sizeof(cur), hipMemcpyDeviceToHost));
    CC_HIP_CHECK(e, hipMemcpy(&st, e->d_states + stream, sizeof(st), hipMemcpyDeviceToHost));
    if (next_id)
        *next_id = cur[0] + 1;
    if (floor_column)
        *floor_column = std::max<int64_t>(cur[1], std::max<int64_t>(0, st.first_column));
    if (readable_from)
        *readable_from = cck::held_from(st.first_column, st.clear_done, 0);
    return CC_OK;
}

} // extern "C"
