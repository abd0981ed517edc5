// cc_k_take.h — k_take_plan, k_take_count, k_take_scan, k_take_scan_streams, k_take_write: what was published (or segmented) since the last
// hand-over, of all streams, compacted into 32-byte records in device memory (cc_engine_take_points).
// (part of cc_kernels.h: included there, in order, inside namespace cck)
//
// Read-only on the engine's planes and on StreamState; the only engine state they write is the cursor array, and that only when every record
// fit. The range of a stream is [max(cursor, clear_done, first_column), upper): columns below StreamState::clear_done have been cleared
// physically, everything from there up to first_unpublished (first_unfinished) is what the publishing (segmentation) chain left and nobody
// changes any more — the same bounds k_scatter_info / k_scatter_apply rely on. Counts are integers from __ballot + popcount and every record's
// place follows from two exclusive scans, so the output does not depend on scheduling. Grids are sized by the host from the plan's longest range.
#pragma once

constexpr int TAKE_SCAN_THREADS = 256;
static_assert(sizeof(cc_take_point) == 32 && alignof(cc_take_point) == 4, "a record is two 16-byte stores");
static_assert(sizeof(cc_take_stream) == 48, "include/cc_hip.h: one table entry per stream");

struct TakeCtl
{
    long long total;    // records of all streams
    long long capacity; // of the caller's record array
    int fits;           // total <= capacity and the caller gave a record array: k_take_write writes and moves the cursors
    int pad;
};

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

// =====================================================================================================
// k_take_plan — per stream: the range a take hands over, what was lost in front of it, the stream's error. One thread per stream; the table goes
// to device memory (for the kernels behind this one) and to pinned host memory (the host sizes their grids by the longest range).
// =====================================================================================================
__global__ __launch_bounds__(64) void k_take_plan(Geometry g, const StreamState* __restrict__ states, const long long* __restrict__ cursors, int stage,
                                                  cc_take_stream* __restrict__ plan, cc_take_stream* __restrict__ h_plan)
{
    const int s = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= g.num_streams)
        return;
    const StreamState* st = &states[s];
    const long long cursor = cursors[(size_t) stage * g.num_streams + s];
    const long long first = st->first_column, cleared = st->clear_done;
    const long long upper = stage == CC_TAKE_CLUSTERED ? st->first_unpublished : st->first_unfinished;
    cc_take_stream t;
    t.col_from = t.col_to = cursor;
    t.lost_columns = 0;
    t.first_record = t.n_records = 0;
    t.error = st->error;
    t.pad = 0;
    if (t.error == 0 && first >= 0 && upper >= 0)
    {
        const long long base = cursor > first ? cursor : first; // (columns in front of the stream's first one never existed: not lost)
        long long from = base > cleared ? base : cleared;
        const long long to = upper > from ? upper : from;       // (a cursor that was sought past `upper` stays where it is)
        if (to - from > g.ring_cols)
            from = to - g.ring_cols;                              // (never: the ring holds no more)
        t.col_from = from;
        t.col_to = to;
        t.lost_columns = from - base;
    }
    plan[s] = t;
    h_plan[s] = t;
    __threadfence_system();
}

// is cell ci (row `row` of a column whose pass over the ring has tag `tag`) handed over? view_column's rule for "the cell holds a return"
// (cc_k_publish.h), then the caller's selection
__device__ __forceinline__ bool take_selects(const SP& p, const int ci, const uint16_t tag, const int select, const int cells)
{
    const float d = p.dist[ci];
    if (!(p.gtag[ci] == tag && d == d))
        return false;
    if (select == CC_TAKE_NOT_GROUND)
        return p.ground[ci] != (uint8_t) CC_GP_GROUND;
    if (select == CC_TAKE_WITH_ID)
    {
        const int r = p.root[ci];
        return r >= 0 && r < cells && p.t_cid[r] != 0u;
    }
    return true;
}

// =====================================================================================================
// k_take_count — selected cells per column. grid = (longest range, streams), block = 64: one wavefront per (column, stream), lanes = rows
// (two trips at 128 rows, as k_gather_clusters walks them). counts[s * stride + c] = cells of column col_from + c.
// =====================================================================================================
__global__ __launch_bounds__(64) void k_take_count(Geometry g, Planes P, const cc_take_stream* __restrict__ plan, int select, unsigned* __restrict__ counts,
                                                   int stride)
{
    const int s = (int) blockIdx.y, c = (int) blockIdx.x;
    const long long from = uniform_i64(plan[s].col_from), to = uniform_i64(plan[s].col_to);
    if (c >= to - from || c >= stride)
        return;
    const SP p = stream_ptrs(P, g, s);
    const int R = g.num_rows, RC = g.ring_cols, lane = lane_id();
    const long long gc = from + c;
    const int lc = (int) (gc % RC);
    const uint16_t tag = cell_tag(gc / RC);
    int n = 0;
    for (int r0 = 0; r0 < R; r0 += 64)
    {
        const int row = r0 + lane;
        const bool sel = row < R && take_selects(p, lc * R + row, tag, select, (int) g.cells);
        n += (int) __popcll(__ballot(sel));
    }
    if (lane == 0)
        counts[(size_t) s * stride + c] = (unsigned) n;
}

// =====================================================================================================
// k_take_scan — exclusive scan of a stream's column counts, in place: counts[s * stride + c] becomes the first record of column c relative to
// the stream's slice; the slice's length goes into the plan. grid = streams, block = TAKE_SCAN_THREADS: every thread sums a run of consecutive
// columns, the runs' sums are scanned in LDS, every thread walks its run again.
// =====================================================================================================
__global__ __launch_bounds__(TAKE_SCAN_THREADS) void k_take_scan(cc_take_stream* __restrict__ plan, unsigned* __restrict__ counts, int stride)
{
    __shared__ long long s_buf[TAKE_SCAN_THREADS];
    const int s = (int) blockIdx.x, t = (int) threadIdx.x;
    long long len = plan[s].col_to - plan[s].col_from;
    len = len > stride ? stride : len;
    unsigned* cnt = counts + (size_t) s * stride;
    const long long per = (len + TAKE_SCAN_THREADS - 1) / TAKE_SCAN_THREADS;
    const long long b = (long long) t * per < len ? (long long) t * per : len;
    const long long e = b + per < len ? b + per : len;
    long long sum = 0;
    for (long long i = b; i < e; i++)
        sum += cnt[i];
    long long total;
    long long off = take_block_scan(s_buf, sum, &total);
    for (long long i = b; i < e; i++)
    {
        const unsigned n = cnt[i];
        cnt[i] = (unsigned) off;
        off += n;
    }
    if (t == 0)
        plan[s].n_records = total;
}

// =====================================================================================================
// k_take_scan_streams — exclusive scan of the streams' totals (first_record of every slice), the verdict on the caller's capacity, and the
// finished table to the caller's device array (if any) and to pinned host memory. grid = 1, block = TAKE_SCAN_THREADS.
// =====================================================================================================
__global__ __launch_bounds__(TAKE_SCAN_THREADS) void k_take_scan_streams(int num_streams, cc_take_stream* __restrict__ plan, long long capacity, int have_records,
                                                                         TakeCtl* __restrict__ ctl, cc_take_stream* __restrict__ d_table,
                                                                         cc_take_stream* __restrict__ h_plan, TakeCtl* __restrict__ h_ctl)
{
    __shared__ long long s_buf[TAKE_SCAN_THREADS];
    const int t = (int) threadIdx.x;
    const int per = (num_streams + TAKE_SCAN_THREADS - 1) / TAKE_SCAN_THREADS;
    const int b = t * per < num_streams ? t * per : num_streams;
    const int e = b + per < num_streams ? b + per : num_streams;
    long long sum = 0;
    for (int i = b; i < e; i++)
        sum += plan[i].n_records;
    long long total;
    long long off = take_block_scan(s_buf, sum, &total);
    for (int i = b; i < e; i++)
    {
        cc_take_stream r = plan[i];
        r.first_record = off;
        off += r.n_records;
        plan[i] = r;
        h_plan[i] = r;
        if (d_table)
            d_table[i] = r;
    }
    if (t == 0)
    {
        TakeCtl c;
        c.total = total;
        c.capacity = capacity;
        c.fits = (have_records && total <= capacity) ? 1 : 0;
        c.pad = 0;
        *ctl = c;
        *h_ctl = c;
    }
    __threadfence_system();
}

// =====================================================================================================
// k_take_write — the records. The same walk as k_take_count: a selected lane's record goes to the stream's first record + its column's offset
// + the selected lanes below it (+ the first trip's cells at 128 rows). Nothing is written unless every record fits the caller's array; then
// the wavefront of a stream's first block also moves the stream's cursor to the end of its range. grid = (max(longest range, 1), streams), block = 64.
// =====================================================================================================
__global__ __launch_bounds__(64) void k_take_write(Geometry g, Planes P, const cc_take_stream* __restrict__ plan, const TakeCtl* __restrict__ ctl, int stage,
                                                   int select, const unsigned* __restrict__ counts, int stride, cc_take_point* __restrict__ records,
                                                   long long* __restrict__ cursors)
{
    if (uniform_i32(ctl->fits) == 0)
        return; // (all or nothing)
    const int s = (int) blockIdx.y, c = (int) blockIdx.x;
    const int lane = lane_id();
    const long long from = uniform_i64(plan[s].col_from), to = uniform_i64(plan[s].col_to);
    if (c == 0 && lane == 0 && plan[s].error == 0)
        cursors[(size_t) stage * g.num_streams + s] = to; // (no block of this launch reads the cursors: the ranges come from the plan)
    if (c >= to - from || c >= stride)
        return;
    const SP p = stream_ptrs(P, g, s);
    const int R = g.num_rows, RC = g.ring_cols;
    const long long capacity = uniform_i64(ctl->capacity);
    const long long gc = from + c;
    const int lc = (int) (gc % RC);
    const uint16_t tag = cell_tag(gc / RC);
    long long pos = uniform_i64(plan[s].first_record) + (long long) counts[(size_t) s * stride + c];
    for (int r0 = 0; r0 < R; r0 += 64)
    {
        const int row = r0 + lane;
        const int ci = lc * R + row;
        const bool sel = row < R && take_selects(p, ci, tag, select, (int) g.cells);
        const unsigned long long mask = __ballot(sel);
        if (sel)
        {
            const long long o = pos + __popcll(mask & lanes_below());
            if (o < capacity) // (always, when the verdict was "fits"; an index is checked where it is used)
            {
                const float4 rec = p.sc_rec[ci];
                unsigned id = 0u;
                if (stage == CC_TAKE_CLUSTERED)
                {
                    const int r = p.root[ci];
                    id = (r >= 0 && r < (int) g.cells) ? p.t_cid[r] : 0u;
                }
                uint4 lo, hi;
                lo.x = __float_as_uint(rec.x);
                lo.y = __float_as_uint(rec.y);
                lo.z = __float_as_uint(rec.z);
                lo.w = __float_as_uint(p.dist[ci]);
                hi.x = id;
                hi.y = p.src[ci];
                hi.z = (unsigned) row | ((unsigned) p.ground[ci] << 16) | ((unsigned) p.inten[ci] << 24);
                hi.w = (unsigned) c;
                uint4* out = (uint4*) (records + o);
                out[0] = lo;
                out[1] = hi;
            }
        }
        pos += __popcll(mask);
    }
}
