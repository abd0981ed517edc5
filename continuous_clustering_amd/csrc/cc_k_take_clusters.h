// cc_k_take_clusters.h — k_tc_plan, k_tc_clear, k_tc_mark, k_tc_scan, k_tc_scan_streams, k_tc_write: the clusters finished since the last
// hand-over, of all streams, as 64-byte descriptors and (grouped by cluster) 32-byte point records in device memory
// (cc_engine_take_clusters).
// (part of cc_kernels.h: included there, in order, inside namespace cck)
//
// Read-only on the engine's planes and on StreamState; the only engine state they write is the (ids taken, floor) pair per stream, and that
// only when every descriptor and record fit. Cluster ids are a counter (StreamState::cluster_counter, cc.cpp:939), so "finished since the last
// take" is the id range [next_id, cluster_counter) and a cluster's slot in the aggregate table is id - id_from: no events, no search. A cell
// of a column below first_unfinished belongs to cluster c iff it holds a return (cell_has_return, cc_k_held.h) and the root of its tree is
// finished and carries c (cell_cluster_id) — what k_gather_clusters relies on, also for columns that are not published yet. The columns come from
// held_range, from the stream's floor up to first_unfinished. Counts are integer atomics (one set per column
// and cluster, all order-free); every place in the output follows from exclusive scans, so the output does not depend on scheduling. Grids
// are sized by the host from the plan.
#pragma once

static_assert(sizeof(cc_take_cluster) == 64 && alignof(cc_take_cluster) == 8, "a descriptor is four 16-byte stores");
static_assert(sizeof(cc_take_cluster_stream) == 56, "include/cc_hip.h: one table entry per stream");

constexpr int TC_MAX_IDS = 65536; // ids a take examines per stream (the newest): bounds the aggregate table of an engine nobody took from

struct TcPlan // per stream: what the kernels behind k_tc_plan walk
{
    long long col_from, col_to; // columns [col_from, col_to) are looked at (empty when there is no id to look for)
    long long id_from;          // slot i of the stream stands for id id_from + i
    long long ids_taken;        // the cursor pair after a take that fits
    long long floor;
    int n_ids, base;            // slots [base, base + n_ids) of the aggregate table
};

struct TcSlot // per examined id, 32 bytes
{
    unsigned count;          // members in the range
    int col_min, col_max;    // first / last column with a member, relative to TcPlan::col_from
    int index;               // descriptor index inside the stream's slice, -1: not handed over
    long long first_record;  // inside the stream's slice
    int stream, pad;
};

struct TcCtl
{
    long long clusters, records;                   // of all streams
    long long cluster_capacity, record_capacity;   // of the caller's arrays
    long long total_ids;                           // slots of the aggregate table
    int fits;                                      // k_tc_write writes and moves the cursors
    int pad;
};

// the id of the finished cluster cell ci belongs to, if that id is one of [id_from, id_to); else 0
__device__ __forceinline__ unsigned tc_member_id(const SP& p, const int ci, const uint16_t tag, const int cells, const long long id_from, const long long id_to)
{
    if (!cell_has_return(p, ci, tag))
        return 0u;
    const int r = cell_root(p, ci, cells);
    if (r < 0 || !p.t_finished[r])
        return 0u;
    const unsigned id = cell_cluster_id(p, ci, cells);
    return ((long long) id >= id_from && (long long) id < id_to) ? id : 0u;
}

// =====================================================================================================
// k_tc_plan — per stream: the ids and the columns a take examines, what was lost in front of them, the stream's error, and the stream's base in
// the aggregate table (an exclusive scan of the id counts). grid = 1, block = TAKE_SCAN_THREADS, every thread a run of consecutive streams.
// The plan goes to device memory and to pinned host memory (the host sizes the grids and the table from it).
// =====================================================================================================
__global__ __launch_bounds__(TAKE_SCAN_THREADS) void k_tc_plan(Geometry g, const StreamState* __restrict__ states, const long long* __restrict__ cursors,
                                                               TcPlan* __restrict__ plan, cc_take_cluster_stream* __restrict__ table,
                                                               TcPlan* __restrict__ h_plan, TcCtl* __restrict__ h_ctl)
{
    __shared__ long long s_buf[TAKE_SCAN_THREADS];
    const int S = g.num_streams, t = (int) threadIdx.x;
    long long b, e;
    run_of(t, S, &b, &e);
    long long sum = 0;
    for (long long s = b; s < e; s++)
    {
        const StreamState* st = &states[s];
        const long long taken = cursors[2 * s], floor = cursors[2 * s + 1];
        const long long first = st->first_column, cleared = st->clear_done, counter = (long long) st->cluster_counter;
        TcPlan pl;
        cc_take_cluster_stream r;
        pl.ids_taken = taken;
        pl.floor = floor;
        pl.id_from = taken + 1;
        pl.col_from = pl.col_to = floor;
        pl.n_ids = pl.base = 0;
        r.lost_columns = r.first_record = r.n_records = 0;
        r.first_cluster = r.n_clusters = 0;
        r.error = st->error;
        r.pad = 0;
        long long id_to = pl.id_from;
        if (r.error == 0 && first >= 0 && st->ring_end >= 0)
        {
            id_to = counter > pl.id_from ? counter : pl.id_from;
            if (id_to - pl.id_from > TC_MAX_IDS)
                pl.id_from = id_to - TC_MAX_IDS; // (an engine nobody took from for thousands of clusters: the newest)
            pl.n_ids = (int) (id_to - pl.id_from);
            // (columns from first_unfinished up have not been associated: their cells' roots are what the previous pass over the ring left, and no
            // finished cluster reaches them — view_column's rule for a cell's id)
            const long long upper = st->first_unfinished < st->ring_end + 1 ? st->first_unfinished : st->ring_end + 1;
            const HeldRange hr = held_range(first, cleared, upper, floor, g.ring_cols);
            r.lost_columns = hr.lost;
            pl.col_from = hr.from;
            pl.col_to = pl.n_ids > 0 ? hr.to : hr.from;             // (no id to look for: no column to walk)
            pl.ids_taken = id_to - 1;
            pl.floor = st->first_unpublished > floor ? st->first_unpublished : floor;
        }
        r.id_from = pl.id_from;
        r.id_to = id_to;
        plan[s] = pl;
        table[s] = r;
        sum += pl.n_ids;
    }
    long long total;
    long long off = take_block_scan(s_buf, sum, &total);
    for (long long s = b; s < e; s++)
    {
        plan[s].base = (int) off; // (the host refuses a total beyond INT_MAX before any kernel uses a base)
        off += plan[s].n_ids;
        h_plan[s] = plan[s];
    }
    if (t == 0)
        h_ctl->total_ids = total;
    __threadfence_system();
}

// =====================================================================================================
// k_tc_clear — the aggregate table's slots of this take. grid = (ceil(longest id range / TAKE_SCAN_THREADS), streams).
// =====================================================================================================
__global__ __launch_bounds__(TAKE_SCAN_THREADS) void k_tc_clear(const TcPlan* __restrict__ plan, TcSlot* __restrict__ slots, long long n_slots)
{
    const int s = (int) blockIdx.y, i = (int) (blockIdx.x * TAKE_SCAN_THREADS + threadIdx.x);
    const long long o = (long long) plan[s].base + i;
    if (i >= plan[s].n_ids || o >= n_slots)
        return;
    TcSlot z;
    z.count = 0u;
    z.col_min = 0x7fffffff;
    z.col_max = -1;
    z.index = -1;
    z.first_record = 0;
    z.stream = s;
    z.pad = 0;
    slots[o] = z;
}

// =====================================================================================================
// k_tc_mark — members per cluster and the columns they span. grid = (longest column range, streams), block = 64: one wavefront per
// (column, stream), lanes = rows (two trips at 128 rows). For every DISTINCT id among the lanes one elected lane adds the id's lanes to the
// cluster's count and folds the column into its span: one set of integer atomics per (column, cluster, trip), not per point; add, min and max
// are order-free.
// =====================================================================================================
__global__ __launch_bounds__(64) void k_tc_mark(Geometry g, Planes P, const TcPlan* __restrict__ plan, const cc_take_cluster_stream* __restrict__ table,
                                                TcSlot* __restrict__ slots, long long n_slots)
{
    HeldColumn h;
    if (!held_column(g, P, plan, 0x7fffffff, &h)) // (no per-stream array: the slots go by id)
        return;
    const int s = h.s, c = h.c;
    const long long id_from = uniform_i64(table[s].id_from), id_to = uniform_i64(table[s].id_to);
    const int base = uniform_i32(plan[s].base), n_ids = uniform_i32(plan[s].n_ids);
    const int R = g.num_rows, lane = lane_id();
    for (int r0 = 0; r0 < R; r0 += 64)
    {
        const int row = r0 + lane;
        const unsigned id = row < R ? tc_member_id(h.p, h.lc * R + row, h.tag, (int) g.cells, id_from, id_to) : 0u;
        unsigned long long todo = __ballot(id != 0u);
        while (todo)
        {
            const int leader = (int) __ffsll((long long) todo) - 1;
            const unsigned that = (unsigned) __builtin_amdgcn_readlane((int) id, leader);
            const unsigned long long same = __ballot(id == that);
            const long long k = (long long) that - id_from;
            if (lane == leader && k >= 0 && k < n_ids && base + k < n_slots)
            {
                TcSlot* sl = &slots[base + k];
                atomicAdd(&sl->count, (unsigned) __popcll(same));
                atomicMin(&sl->col_min, c);
                atomicMax(&sl->col_max, c);
            }
            todo &= ~same;
        }
    }
}

// =====================================================================================================
// k_tc_scan — per stream: which of its ids are handed over (count >= min_points, and at least one member), their descriptor index and first
// record inside the stream's slices (two exclusive scans), the slices' lengths into the table. grid = streams, block = TAKE_SCAN_THREADS.
// =====================================================================================================
__global__ __launch_bounds__(TAKE_SCAN_THREADS) void k_tc_scan(const TcPlan* __restrict__ plan, cc_take_cluster_stream* __restrict__ table,
                                                               TcSlot* __restrict__ slots, long long n_slots, unsigned min_points)
{
    __shared__ long long s_buf[TAKE_SCAN_THREADS];
    const int s = (int) blockIdx.x, t = (int) threadIdx.x;
    const unsigned need = min_points > 1u ? min_points : 1u;
    long long len = plan[s].n_ids;
    len = plan[s].base + len > n_slots ? n_slots - plan[s].base : len;
    len = len > 0 ? len : 0;
    TcSlot* sl = slots + plan[s].base;
    long long b, e;
    run_of(t, len, &b, &e);
    long long n_keep = 0, n_rec = 0;
    for (long long i = b; i < e; i++)
        if (sl[i].count >= need)
        {
            n_keep++;
            n_rec += sl[i].count;
        }
    long long total_keep, total_rec;
    long long k = take_block_scan(s_buf, n_keep, &total_keep);
    long long o = take_block_scan(s_buf, n_rec, &total_rec);
    for (long long i = b; i < e; i++)
        if (sl[i].count >= need)
        {
            sl[i].index = (int) k++;
            sl[i].first_record = o;
            o += sl[i].count;
        }
    if (t == 0)
    {
        table[s].n_clusters = (int) total_keep;
        table[s].n_records = total_rec;
    }
}

// =====================================================================================================
// k_tc_scan_streams — exclusive scans of the streams' totals (first_cluster and first_record of every slice), the verdict on the caller's
// capacities, and the finished table to the caller's device array (if any) and to pinned host memory. grid = 1, block = TAKE_SCAN_THREADS.
// =====================================================================================================
__global__ __launch_bounds__(TAKE_SCAN_THREADS) void k_tc_scan_streams(int num_streams, cc_take_cluster_stream* __restrict__ table, long long cluster_capacity,
                                                                       long long record_capacity, int have_clusters, int need_records, long long total_ids,
                                                                       TcCtl* __restrict__ ctl, cc_take_cluster_stream* __restrict__ d_table,
                                                                       cc_take_cluster_stream* __restrict__ h_table, TcCtl* __restrict__ h_ctl)
{
    __shared__ long long s_buf[TAKE_SCAN_THREADS];
    const int t = (int) threadIdx.x;
    long long b, e;
    run_of(t, num_streams, &b, &e);
    long long n_cl = 0, n_rec = 0;
    for (long long i = b; i < e; i++)
    {
        n_cl += table[i].n_clusters;
        n_rec += table[i].n_records;
    }
    long long total_cl, total_rec;
    long long k = take_block_scan(s_buf, n_cl, &total_cl);
    long long o = take_block_scan(s_buf, n_rec, &total_rec);
    for (long long i = b; i < e; i++)
    {
        cc_take_cluster_stream r = table[i];
        r.first_cluster = (int) k;
        r.first_record = o;
        k += r.n_clusters;
        o += r.n_records;
        table[i] = r;
        h_table[i] = r;
        if (d_table)
            d_table[i] = r;
    }
    if (t == 0)
    {
        TcCtl c;
        c.clusters = total_cl;
        c.records = total_rec;
        c.cluster_capacity = cluster_capacity;
        c.record_capacity = record_capacity;
        c.total_ids = total_ids;
        c.fits = (have_clusters && total_cl <= cluster_capacity && total_cl <= 0x7fffffffll && (!need_records || total_rec <= record_capacity)) ? 1 : 0;
        c.pad = 0;
        *ctl = c;
        *h_ctl = c;
    }
    __threadfence_system();
}

// =====================================================================================================
// k_tc_write — descriptors and records. grid = streams + examined ids, block = 64. Nothing happens unless everything fits the caller's arrays.
// Block s < streams moves the cursor pair of stream s (no block of this launch reads the cursors: everything comes from the plan). Block
// streams + j is slot j of the aggregate table: one wavefront per cluster, the others return. It walks the cluster's columns as
// k_gather_clusters does — a member's record goes to the cluster's first record + the members met so far + the member lanes below it — with
// the record assembled in registers and stored as two 16-byte stores, keeps the bounding box and the firing range in registers, reduces them
// over the wavefront at the end, and lane 0 stores the descriptor (four 16-byte stores). records == nullptr: descriptors only.
// =====================================================================================================
__global__ __launch_bounds__(64) void k_tc_write(Geometry g, Planes P, const TcPlan* __restrict__ plan, const cc_take_cluster_stream* __restrict__ table,
                                                 const TcCtl* __restrict__ ctl, const TcSlot* __restrict__ slots, long long n_slots,
                                                 cc_take_cluster* __restrict__ clusters, cc_take_point* __restrict__ records, long long* __restrict__ cursors)
{
    if (uniform_i32(ctl->fits) == 0)
        return; // (all or nothing)
    const int S = g.num_streams, lane = lane_id();
    if ((int) blockIdx.x < S)
    {
        const int s = (int) blockIdx.x;
        if (lane == 0 && table[s].error == 0)
        {
            cursors[2 * s] = plan[s].ids_taken;
            cursors[2 * s + 1] = plan[s].floor;
        }
        return;
    }
    const long long j = (long long) blockIdx.x - S;
    if (j >= n_slots)
        return;
    const TcSlot sl = slots[j];
    const int index = uniform_i32(sl.index), s = uniform_i32(sl.stream);
    if (index < 0 || s < 0 || s >= S)
        return;
    const int col_min = uniform_i32(sl.col_min), col_max = uniform_i32(sl.col_max);
    const unsigned count = (unsigned) uniform_i32((int) sl.count);
    const TcPlan pl = plan[s];
    const long long from = uniform_i64(pl.col_from);
    const unsigned id = (unsigned) (uniform_i64(pl.id_from) + (j - uniform_i32(pl.base)));
    const long long d_index = (long long) uniform_i32(table[s].first_cluster) + index;
    const long long first = uniform_i64(table[s].first_record) + uniform_i64(sl.first_record);
    const long long cluster_capacity = uniform_i64(ctl->cluster_capacity), record_capacity = uniform_i64(ctl->record_capacity);
    if (col_min < 0 || col_max < col_min || col_max >= g.ring_cols || d_index >= cluster_capacity)
        return; // (never: the verdict was "fits" and k_tc_mark only folds columns of the range)
    const SP p = stream_ptrs(P, g, s);
    const int R = g.num_rows, RC = g.ring_cols;
    const long long end = first + count;
    long long pos = first;
    float lo_x = __int_as_float(0x7f800000), lo_y = lo_x, lo_z = lo_x, hi_x = -lo_x, hi_y = -lo_x, hi_z = -lo_x;
    unsigned f_min = 0xffffffffu, f_max = 0u;
    const long long gc0 = from + col_min;
    int lc = (int) (gc0 % RC);
    long long pass = gc0 / RC;
    for (int c = col_min; c <= col_max; c++)
    {
        const uint16_t tag = cell_tag(pass);
        for (int r0 = 0; r0 < R; r0 += 64)
        {
            const int row = r0 + lane;
            const int ci = lc * R + row;
            const bool mine = row < R && tc_member_id(p, ci, tag, (int) g.cells, (long long) id, (long long) id + 1) == id;
            const unsigned long long mask = __ballot(mine);
            if (mine)
            {
                const float4 rec = p.sc_rec[ci];
                const unsigned src = p.src[ci];
                lo_x = rec.x < lo_x ? rec.x : lo_x;
                lo_y = rec.y < lo_y ? rec.y : lo_y;
                lo_z = rec.z < lo_z ? rec.z : lo_z;
                hi_x = rec.x > hi_x ? rec.x : hi_x;
                hi_y = rec.y > hi_y ? rec.y : hi_y;
                hi_z = rec.z > hi_z ? rec.z : hi_z;
                f_min = src < f_min ? src : f_min;
                f_max = src > f_max ? src : f_max;
                const long long o = pos + __popcll(mask & lanes_below());
                if (records && o < end && o < record_capacity) // (always, when the verdict was "fits"; an index is checked where it is used)
                    store_take_point(records + o, p, ci, row, id, (unsigned) (c - col_min));
            }
            pos += __popcll(mask);
        }
        if (++lc == RC)
        {
            lc = 0;
            pass++;
        }
    }
    // (all 64 lanes are here: the reductions need them)
    lo_x = wave_min_f32(lo_x);
    lo_y = wave_min_f32(lo_y);
    lo_z = wave_min_f32(lo_z);
    hi_x = wave_max_f32(hi_x);
    hi_y = wave_max_f32(hi_y);
    hi_z = wave_max_f32(hi_z);
    f_min = wave_min_u32(f_min);
    f_max = wave_max_u32(f_max);
    if (lane == 0)
    {
        const long long col_from = from + col_min;
        uint4 q0, q1, q2, q3;
        q0.x = (unsigned) s;
        q0.y = id;
        q0.z = (unsigned) (unsigned long long) col_from;
        q0.w = (unsigned) ((unsigned long long) col_from >> 32);
        q1.x = (unsigned) (unsigned long long) first;
        q1.y = (unsigned) ((unsigned long long) first >> 32);
        q1.z = count;
        q1.w = (unsigned) (col_max - col_min + 1);
        q2.x = f_min;
        q2.y = f_max;
        q2.z = __float_as_uint(lo_x);
        q2.w = __float_as_uint(lo_y);
        q3.x = __float_as_uint(lo_z);
        q3.y = __float_as_uint(hi_x);
        q3.z = __float_as_uint(hi_y);
        q3.w = __float_as_uint(hi_z);
        uint4* out = (uint4*) (clusters + d_index);
        out[0] = q0;
        out[1] = q1;
        out[2] = q2;
        out[3] = q3;
    }
}
