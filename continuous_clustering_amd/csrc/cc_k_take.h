// cc_k_take.h — k_take_plan, k_take_count, k_take_scan, k_take_scan_streams, k_take_write: what was published (or segmented) since the last
// hand-over, of all streams, compacted into 32-byte records in device memory (cc_engine_take_points).
// (part of cc_kernels.h: included there, in order, inside namespace cck)
//
// Read-only on the engine's planes and on StreamState; the only engine state they write is the cursor array, and that only when every record
// fit. The range of a stream is held_range (cc_k_held.h) from the stream's cursor up to first_unpublished (first_unfinished). Counts are
// integers from __ballot + popcount and every record's place follows from two exclusive scans (run_of, take_block_scan), so the output does not
// depend on scheduling. Grids are sized by the host from the plan's longest range.
#pragma once

static_assert(sizeof(cc_take_stream) == 48, "include/cc_hip.h: one table entry per stream");

struct TakeCtl
{
    long long total;    // records of all streams
    long long capacity; // of the caller's record array
    int fits;           // total <= capacity and the caller gave a record array: k_take_write writes and moves the cursors
    int pad;
};

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
    const long long first = st->first_column;
    const long long upper = stage == CC_TAKE_CLUSTERED ? st->first_unpublished : st->first_unfinished;
    cc_take_stream t;
    t.col_from = t.col_to = cursor;
    t.lost_columns = 0;
    t.first_record = t.n_records = 0;
    t.error = st->error;
    t.pad = 0;
    if (t.error == 0 && first >= 0 && upper >= 0)
    {
        const HeldRange r = held_range(first, st->clear_done, upper, cursor, g.ring_cols);
        t.col_from = r.from;
        t.col_to = r.to;
        t.lost_columns = r.lost;
    }
    plan[s] = t;
    h_plan[s] = t;
    __threadfence_system();
}

// is cell ci (row `row` of a column whose pass over the ring has tag `tag`) handed over? It holds a return, then the caller's selection
__device__ __forceinline__ bool take_selects(const SP& p, const int ci, const uint16_t tag, const int select, const int cells)
{
    if (!cell_has_return(p, ci, tag))
        return false;
    if (select == CC_TAKE_NOT_GROUND)
        return p.ground[ci] != (uint8_t) CC_GP_GROUND;
    if (select == CC_TAKE_WITH_ID)
        return cell_cluster_id(p, ci, cells) != 0u;
    return true;
}

// =====================================================================================================
// k_take_count — selected cells per column. grid = (longest range, streams), block = 64: one wavefront per (column, stream), lanes = rows
// (two trips at 128 rows, as k_gather_clusters walks them). counts[s * stride + c] = cells of column col_from + c.
// =====================================================================================================
__global__ __launch_bounds__(64) void k_take_count(Geometry g, Planes P, const cc_take_stream* __restrict__ plan, int select, unsigned* __restrict__ counts,
                                                   int stride)
{
    HeldColumn h;
    if (!held_column(g, P, plan, stride, &h))
        return;
    const int R = g.num_rows, lane = lane_id();
    int n = 0;
    for (int r0 = 0; r0 < R; r0 += 64)
    {
        const int row = r0 + lane;
        const bool sel = row < R && take_selects(h.p, h.lc * R + row, h.tag, select, (int) g.cells);
        n += (int) __popcll(__ballot(sel));
    }
    if (lane == 0)
        counts[(size_t) h.s * stride + h.c] = (unsigned) n;
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
    long long b, e;
    run_of(t, len, &b, &e);
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
    long long b, e;
    run_of(t, num_streams, &b, &e);
    long long sum = 0;
    for (long long i = b; i < e; i++)
        sum += plan[i].n_records;
    long long total;
    long long off = take_block_scan(s_buf, sum, &total);
    for (long long i = b; i < e; i++)
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
    const int s = (int) blockIdx.y;
    const int lane = lane_id();
    if (blockIdx.x == 0 && lane == 0 && plan[s].error == 0)
        cursors[(size_t) stage * g.num_streams + s] = plan[s].col_to; // (no block of this launch reads the cursors: the ranges come from the plan)
    HeldColumn h;
    if (!held_column(g, P, plan, stride, &h))
        return;
    const SP& p = h.p;
    const int R = g.num_rows;
    const long long capacity = uniform_i64(ctl->capacity);
    long long pos = uniform_i64(plan[s].first_record) + (long long) counts[(size_t) s * stride + h.c];
    for (int r0 = 0; r0 < R; r0 += 64)
    {
        const int row = r0 + lane;
        const int ci = h.lc * R + row;
        const bool sel = row < R && take_selects(p, ci, h.tag, select, (int) g.cells);
        const unsigned long long mask = __ballot(sel);
        if (sel)
        {
            const long long o = pos + __popcll(mask & lanes_below());
            if (o < capacity) // (always, when the verdict was "fits"; an index is checked where it is used)
                store_take_point(records + o, p, ci, row, stage == CC_TAKE_CLUSTERED ? cell_cluster_id(p, ci, (int) g.cells) : 0u, (unsigned) h.c);
        }
        pos += __popcll(mask);
    }
}
