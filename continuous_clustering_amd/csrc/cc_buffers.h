// cc_buffers.h — who owns the engine's memory besides the planes: the grow-only device scratch (one function per buffer), the pinned host blocks
// (a registry with two lifetimes) and the lists of streams and events. Host code only. Not a header of its own: cc_engine.hip includes it once,
// inside its anonymous namespace, behind cc_engine, CC_HIP_CHECK and alloc_plane and in front of cc_launch.h.

// ---- grow-only device scratch ------------------------------------------------------------------------------------------------------------------
// Nothing when `*capacity` covers `need`; else a new block of `new_capacity` elements. The old block stays in `allocations` until the engine is
// destroyed or re-shaped (free_all): captured small-call graphs and kernels in flight may still hold it, and growth is rare (sizes repeat).
// Outside allocate() alloc_plane is a plain hipMalloc: none of this scratch is part of the slab.
template<class T>
int grow_scratch(cc_engine* e, T** ptr, size_t* capacity, size_t need, size_t new_capacity)
{
    if (*capacity >= need)
        return CC_OK;
    int rc = alloc_plane(e, ptr, new_capacity);
    if (rc)
        return rc;
    *capacity = new_capacity;
    return CC_OK;
}

// the per-firing ego records of the four batch-descriptor slots, for `need` firings (streams in launch x n)
static int ensure_ego(cc_engine* e, size_t need)
{
    if (e->ego_capacity < need)
    {
        const size_t cap = need < 4096 ? 4096 : need;
        for (double*& p : e->d_ego)
        {
            size_t none = 0; // (one capacity for the four blocks: set below, once all of them are there)
            int rc = grow_scratch(e, &p, &none, cap * cck::EGO_STRIDE, cap * cck::EGO_STRIDE);
            if (rc)
                return rc;
        }
        e->ego_capacity = cap;
        e->small_graphs_stale = true; // captured small-call graphs bake the old pointers
    }
    return CC_OK;
}

// ---- pinned host blocks ------------------------------------------------------------------------------------------------------------------------
// Every hipHostMalloc block of the engine is allocated here, which records where its pointer lives and how long it lives:
//   PIN_SHAPE   sized for the row count or tied to the planes of the current shape: freed by free_all (cc_engine_reset to another shape, destroy)
//   PIN_ENGINE  as long as the engine: freed by cc_engine_destroy and by the failure path of cc_engine_create
enum PinnedLifetime { PIN_SHAPE, PIN_ENGINE };

template<class T>
void release_pinned(T** slot)
{
    if (*slot)
        (void) hipHostFree(*slot);
    *slot = nullptr;
}

// (a block that exists is freed first: the caller wants another size)
template<class T>
int alloc_pinned(cc_engine* e, T** slot, size_t bytes, PinnedLifetime lifetime)
{
    release_pinned(slot);
    const hipError_t err = hipHostMalloc((void**) slot, bytes);
    if (err != hipSuccess)
    {
        *slot = nullptr;
        e->error = std::string("hipHostMalloc: ") + hipGetErrorString(err);
        return CC_ERR_HIP;
    }
    const std::pair<void**, int> rec{(void**) slot, (int) lifetime};
    if (std::find(e->pinned.begin(), e->pinned.end(), rec) == e->pinned.end())
        e->pinned.push_back(rec);
    return CC_OK;
}

static void free_pinned(cc_engine* e, PinnedLifetime lifetime)
{
    for (const auto& rec : e->pinned)
        if (rec.second == (int) lifetime)
            release_pinned(rec.first);
}

// the staging of cc_engine_read_columns: a device block and its pinned mirror (one D2H copy per read)
static int ensure_view(cc_engine* e, size_t bytes)
{
    int rc = grow_scratch(e, &e->d_view, &e->view_bytes, bytes, bytes);
    if (rc)
        return rc;
    if (e->h_view_bytes < bytes)
    {
        e->h_view_bytes = 0;
        if ((rc = alloc_pinned(e, &e->h_view, bytes, PIN_ENGINE)))
            return rc;
        e->h_view_bytes = bytes;
    }
    return CC_OK;
}

// the scratch of cc_engine_gather_cluster_points and cc_engine_scatter_info (a hipMalloc / hipFree pair per call costs more than the gather):
// the queries take twice what they need, so that requests that creep up do not re-allocate call after call
static int ensure_gather(cc_engine* e, size_t need, size_t headroom = 2)
{
    return e->gather_bytes < need ? grow_scratch(e, &e->d_gather, &e->gather_bytes, need, need * headroom) : CC_OK;
}

// ---- streams and events ------------------------------------------------------------------------------------------------------------------------
// fn(hipStream_t) -> int over the engine's six streams, `stream` first; stops at the first non-zero result and returns it
template<class F>
int for_each_stream(cc_engine* e, F fn)
{
    for (hipStream_t s : {e->stream, e->stream2, e->stream3, e->stream4, e->stream5, e->stream6})
    {
        int rc = fn(s);
        if (rc)
            return rc;
    }
    return CC_OK;
}

static int sync_streams(cc_engine* e)
{
    return for_each_stream(e, [e](hipStream_t s) -> int
    {
        CC_HIP_CHECK(e, hipStreamSynchronize(s));
        return CC_OK;
    });
}

// fn(hipEvent_t&) over every event the engine creates with itself (the pools of timing events grow on demand and are apart)
template<class F>
void for_each_event(cc_engine* e, F fn)
{
    for (hipEvent_t* group : {e->ev_ins, e->ev_gate, e->ev_seg, e->ev_assoc, e->ev_segscan, e->ev_prep, e->ev_pubrdy})
        for (int i = 0; i < 4; i++)
            fn(group[i]);
    for (hipEvent_t& ev : e->ev_rel)
        fn(ev);
    fn(e->ev_input);
}
