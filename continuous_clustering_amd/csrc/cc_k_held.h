// cc_k_held.h — what a reader of the columns a stream still holds needs: the range it may look at (held_range / held_from), the column of a
// block of a launch over such ranges (HeldColumn), the rules for a cell's return and cluster id, the 32-byte point record, and the block scan
// that places compacted output. Used by the id backlog (cc_k_publish.h), the takes (cc_k_take.h, cc_k_take_clusters.h), the frame scatter and the
// replay evaluator (cc_k_replay_eval.h), and by the host's cursor queries (cc_take.h). DESIGN.md section 15.
// (part of cc_kernels.h: included there, in order, inside namespace cck. The range rule is plain C++ without HIP types: a host-only program that
// defines CC_HELD_RANGE_ONLY gets held_range, held_from and the range of an image take, image_range, alone — tests/csrc/held_range_probe.cpp,
// tests/csrc/image_range_probe.cpp)
#pragma once

#if defined(__HIPCC__)
#define CC_HELD_FN __host__ __device__ inline
#else
#define CC_HELD_FN inline
#endif

// ---- the range --------------------------------------------------------------------------------------------------------------------------
// Columns below StreamState::clear_done have been cleared physically (clearing lags ring_start by a batch, so what a call published stays
// readable behind ring_start); columns in front of StreamState::first_column never existed. From there up to `upper` — first_unpublished for
// what the publishing chain left, first_unfinished for what the segmentation left — nobody changes a cell any more.
struct HeldRange
{
    long long from, to; // the columns [from, to) may be read
    long long lost;     // columns between the reader's cursor and `from` that existed once and are gone
};

// the lowest column a reader at `cursor` may still look at
CC_HELD_FN long long held_from(const long long first_column, const long long clear_done, const long long cursor)
{
    const long long base = cursor > first_column ? cursor : first_column;
    return base > clear_done ? base : clear_done;
}

// for a stream that has started (first_column >= 0, upper >= 0: the callers test that, and the stream's error)
CC_HELD_FN HeldRange held_range(const long long first_column, const long long clear_done, const long long upper, const long long cursor, const long long ring_cols)
{
    const long long base = cursor > first_column ? cursor : first_column; // (columns in front of the stream's first one never existed: not lost)
    HeldRange r;
    r.from = held_from(first_column, clear_done, cursor);
    r.to = upper > r.from ? upper : r.from; // (a cursor that was sought past `upper` stays where it is)
    if (r.to - r.from > ring_cols)
        r.from = r.to - ring_cols;          // (never: the ring holds no more)
    r.lost = r.from - base;
    return r;
}

// ---- the range of a reader that hands held columns over as whole rotations -----------------------------------------------------------------
// For a reader that writes rotations of W columns into a ring of `slots` row-major images, rotation r into slot r % slots (no kernel does
// yet: this is the range rule alone, checked by tests/test_take_images_cpu.py). Such a take writes whole columns [from, to): empty below
// `readable_from`, from the engine's ring from there on.
struct ImageRange
{
    long long from, to;                   // the columns [from, to) are written
    long long readable_from;              // the first of them that comes from the ring (== to: none does)
    long long lost;                       // HeldRange::lost
    long long skipped;                    // readable columns dropped because the image ring holds `slots` rotations only
    long long rotation_from, rotation_to; // the rotations [rotation_from, rotation_to) get their last column
};

// for a stream that has started, as held_range (one that has not yields an empty range at the cursor)
CC_HELD_FN ImageRange image_range(const long long first_column, const long long clear_done, const long long upper, const long long cursor, const long long ring_cols,
                                  const long long W, const long long slots)
{
    const HeldRange h = held_range(first_column, clear_done, upper, cursor, ring_cols);
    const long long a0 = first_column / W * W; // (the first rotation's columns in front of the stream's first one never existed: written empty, not lost)
    const long long c1 = cursor > a0 ? cursor : a0;
    const long long rot_of_from = h.from / W * W; // (a rotation the cursor stands in is abandoned when clearing has reached a later one)
    long long start = c1 > rot_of_from ? c1 : rot_of_from;
    const long long oldest = (h.to / W - (slots - 1)) * W; // the image ring holds the rotation of h.to and slots - 1 before it
    ImageRange r;
    r.skipped = 0;
    if (start < oldest)
    {
        const long long readable = start > h.from ? start : h.from;
        r.skipped = oldest > readable ? oldest - readable : 0;
        start = oldest;
    }
    r.from = start;
    r.to = h.to;
    r.readable_from = start > h.from ? start : h.from;
    r.lost = h.lost;
    r.rotation_from = start / W;
    r.rotation_to = h.to / W > r.rotation_from ? h.to / W : r.rotation_from;
    return r;
}

// of the columns [from, to) an image take writes, those inside rotation `rot`: how many, and how many of them are written empty because they
// had been cleared (at or above the stream's first column, below readable_from)
CC_HELD_FN void image_rotation_share(const ImageRange& r, const long long first_column, const long long rot, const long long W, long long* written, long long* lost)
{
    const long long lo = rot * W, hi = lo + W;
    const long long a = r.from > lo ? r.from : lo, b = r.to < hi ? r.to : hi;
    *written = b > a ? b - a : 0;
    const long long la = a > first_column ? a : first_column, lb = b < r.readable_from ? b : r.readable_from;
    *lost = lb > la ? lb - la : 0;
}

#ifndef CC_HELD_RANGE_ONLY

static_assert(sizeof(cc_take_point) == 32 && alignof(cc_take_point) == 4, "a record is two 16-byte stores");

// ---- a launch over the ranges of all streams: grid = (longest range, streams), block = 64 -------------------------------------------------
struct HeldColumn
{
    int s, c;     // stream (blockIdx.y), column relative to the range's first (blockIdx.x)
    long long gc; // global column
    int lc;       // its ring slot
    uint16_t tag; // of its pass over the ring
    SP p;
};

// the column of this block in the range [col_from, col_to) its stream's plan entry names (cc_take_stream, TcPlan, cc_replay_stream); false: the
// block has none (beyond the range, or beyond a per-stream array of `stride` entries)
template<class PlanEntry>
__device__ __forceinline__ bool held_column(const Geometry& g, const Planes& P, const PlanEntry* plan, const int stride, HeldColumn* h)
{
    h->s = (int) blockIdx.y;
    h->c = (int) blockIdx.x;
    const long long from = uniform_i64(plan[h->s].col_from), to = uniform_i64(plan[h->s].col_to);
    if (h->c >= to - from || h->c >= stride)
        return false;
    h->p = stream_ptrs(P, g, h->s);
    h->gc = from + h->c;
    h->lc = (int) (h->gc % g.ring_cols);
    h->tag = cell_tag(h->gc / g.ring_cols);
    return true;
}

// ---- a cell -----------------------------------------------------------------------------------------------------------------------------
// "the cell holds a return of this pass": view_column's rule (cc_k_publish.h) — ring-pass tag matches and distance is not NaN
__device__ __forceinline__ bool cell_has_return(const SP& p, const int ci, const uint16_t tag)
{
    const float d = p.dist[ci];
    return p.gtag[ci] == tag && d == d;
}

// The frame scatter's rule is a different one: the distance alone, without the tag, for a column the caller knows to lie inside
// [clear_done, first_unpublished). The two probably agree on every reachable state, but nobody has shown it, so they stay apart.
__device__ __forceinline__ bool scatter_cell_has_return(const SP& p, const int ci)
{
    return p.dist[ci] == p.dist[ci];
}

// the root cell of ci's tree, -1: none
__device__ __forceinline__ int cell_root(const SP& p, const int ci, const int cells)
{
    const int r = p.root[ci];
    return (r >= 0 && r < cells) ? r : -1;
}

// the id of the cluster cell ci belongs to (0: none), read from the tree's root — not from Planes::id, which is only kept once a caller has asked for it
__device__ __forceinline__ unsigned cell_cluster_id(const SP& p, const int ci, const int cells)
{
    const int r = cell_root(p, ci, cells);
    return r >= 0 ? p.t_cid[r] : 0u;
}

// cc_take_point (include/cc_hip.h) of cell ci, assembled in registers, as two 16-byte stores
__device__ __forceinline__ void store_take_point(cc_take_point* out, const SP& p, const int ci, const int row, const unsigned id, const unsigned rel_col)
{
    const float4 rec = p.sc_rec[ci];
    uint4 lo, hi;
    lo.x = __float_as_uint(rec.x);
    lo.y = __float_as_uint(rec.y);
    lo.z = __float_as_uint(rec.z);
    lo.w = __float_as_uint(p.dist[ci]);
    hi.x = id;
    hi.y = p.src[ci];
    hi.z = (unsigned) row | ((unsigned) p.ground[ci] << 16) | ((unsigned) p.inten[ci] << 24);
    hi.w = rel_col;
    uint4* o = (uint4*) out;
    o[0] = lo;
    o[1] = hi;
}

// ---- placing compacted output: every thread of a block takes a run of consecutive items, the runs' sums are scanned ---------------------------
constexpr int TAKE_SCAN_THREADS = 256;

// thread t's run [*b, *e) of n items
__device__ __forceinline__ void run_of(const int t, const long long n, long long* b, long long* e)
{
    const long long per = (n + TAKE_SCAN_THREADS - 1) / TAKE_SCAN_THREADS;
    *b = (long long) t * per < n ? (long long) t * per : n;
    *e = *b + per < n ? *b + per : n;
}

// exclusive scan of one value per thread over a block of TAKE_SCAN_THREADS threads (Hillis-Steele in LDS); *total = the sum, to every thread
__device__ __forceinline__ long long take_block_scan(long long* s_buf, const long long v, long long* total)
{
    const int t = (int) threadIdx.x;
    s_buf[t] = v;
    __syncthreads();
    for (int d = 1; d < TAKE_SCAN_THREADS; d <<= 1)
    {
        const long long add = t >= d ? s_buf[t - d] : 0ll;
        __syncthreads();
        s_buf[t] += add;
        __syncthreads();
    }
    const long long incl = s_buf[t];
    *total = s_buf[TAKE_SCAN_THREADS - 1];
    __syncthreads(); // (s_buf may be filled again)
    return incl - v;
}

#endif // CC_HELD_RANGE_ONLY
