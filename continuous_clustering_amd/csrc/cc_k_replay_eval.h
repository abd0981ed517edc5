// cc_k_replay_eval.h — the frame scatter of the reference's harness (addColumnAndEvaluateFrameIfCompleted, kitti_demo.cpp:173-224) for one
// stream and a caller's columns (k_scatter_info, k_scatter_apply: cc_engine_scatter_*), and — k_replay_poke, k_replay_plan, k_replay_info,
// k_replay_walk, k_replay_scan, k_replay_apply, k_replay_eval, k_replay_compact — the same scatter and the label compare of the frames it
// completes (kitti_evaluation.cpp:29-146) for ALL streams of a replay engine per call (cc_replay_eval_step, include/cc_kitti.h, DESIGN.md
// section 18).
// (part of cc_kernels.h: included there, in order, inside namespace cck)
//
// Read-only on the engine's planes and on StreamState. The range of a stream is held_range (cc_k_held.h) from the stream's cursor up to
// first_unpublished; grids are sized by the host from the plan's longest range and from the number of completed frames, never from
// ring_cols x streams. Everything is integer: ballots, find-first-set, one exclusive scan over the streams, order-free atomics in the label
// compare (ccev::eval_point, shared with cc_eval_frame_device). The entropies are summed on the host from the exact pair counts.
#pragma once

static_assert(sizeof(cc_replay_stream) == 48, "include/cc_kitti.h: one table entry per stream");
static_assert(sizeof(cc_replay_record) == 56, "include/cc_kitti.h: two int32 and six doubles");

// what the handle keeps per stream between steps (device memory)
struct ReplayState
{
    long long cursor;       // first column the next step looks at
    long long error_column; // of the sticky error
    int prev;               // kitti_demo.cpp previous_frame_index
    int active;
    int error;              // CC_REPLAY_ERR_* raised by a step, kept until cc_replay_eval_seek
    int pad;
};

// what k_replay_walk found for a stream (device memory, read by k_replay_scan and k_replay_apply)
struct ReplayWalk
{
    long long apply_to;     // columns [col_from, apply_to) are applied and leave the cursor behind them
    long long error_column;
    int first_frame;        // completed frames: first_frame .. first_frame + n_done - 1
    int n_done;
    int new_prev;
    int new_active;
    int error;
    int pad;
};

struct ReplayJob
{
    int stream, frame;
};

struct ReplayCtl
{
    long long total;    // completed frames of all streams
    long long capacity; // of the caller's record array
    int fits;
    int pad;
};

// one distinct (ground truth, detection) pair of an evaluation lane: one 16-byte store into pinned host memory
struct ReplayPair
{
    unsigned long long key;
    unsigned count;
    unsigned lane;
};
static_assert(sizeof(ReplayPair) == 16, "one 16-byte store");

constexpr int REPLAY_COUNTS = 8; // unsigned long long per evaluation lane: tp, fn, fp, tn, the pairs that look like a free slot, 3 unused

// slot of frame f (f may be negative after a seek)
__device__ __forceinline__ int replay_slot(const int frame, const int slots)
{
    const int m = frame % slots;
    return m < 0 ? m + slots : m;
}

// =====================================================================================================
// The frame scatter of the reference's harness (addColumnAndEvaluateFrameIfCompleted, kitti_demo.cpp:173-224) for a replayed KITTI sequence, on
// the device. A stream that is fed exactly num_columns pseudo-firings per frame (kitti_demo.cpp:386-403) carries, per cell, the sequence number
// of the firing that filled it: frame = sequence / num_columns, range-image column of the frame = sequence % num_columns, and the KITTI point of
// the cell is original_index[frame % slots][column][row] (cc_kitti_frame::d_original_index of the frame's conversion). Both halves work on ONE
// held column (ring slot lc of stream s) by one wavefront, lanes = rows; the single-stream kernels (cc_engine_scatter_info / _apply) and the
// all-stream kernels (cc_replay_eval_step) below are wrappers that say which column.
// =====================================================================================================
// the smallest / largest frame among the points of the column (INT32_MAX / -1 for a column without points, or one that is not `live`): what the
// harness needs to find where frame N + 1 starts (:205-209), and its two error conditions
__device__ __forceinline__ void scatter_column_info(const Geometry& g, const SP& p, const int s, const int lc, const bool live,
                                                    const int* __restrict__ original_index, const int slots, int* out_min, int* out_max)
{
    const int R = g.num_rows, NC = g.num_columns;
    const int* org = original_index + (size_t) s * (size_t) slots * (size_t) NC * (size_t) R;
    int mn = 0x7fffffff, mx = -1;
    for (int row = lane_id(); live && row < R; row += 64)
    {
        const int ci = lc * R + row;
        if (scatter_cell_has_return(p, ci))
        {
            const unsigned seq = p.src[ci];
            const int frame = (int) (seq / (unsigned) NC), col = (int) (seq % (unsigned) NC);
            if (org[((size_t) (frame % slots) * NC + col) * R + row] >= 0)
            {
                mn = frame < mn ? frame : mn;
                mx = frame > mx ? frame : mx;
            }
        }
    }
    mn = wave_min_i32(mn);
    mx = -wave_min_i32(-mx);
    if (lane_id() == 0)
    {
        *out_min = mn;
        *out_max = mx;
    }
}

// is_ground_point = (ground_point_label == GP_GROUND) and detection_label = id (:214-215) of the column's points into the frames' arrays in
// HBM, which the label compare then reads
__device__ __forceinline__ void scatter_column_apply(const Geometry& g, const SP& p, const int s, const int lc, const int* __restrict__ original_index,
                                                     const int slots, unsigned char* __restrict__ is_ground, unsigned* __restrict__ detection,
                                                     const long long max_points)
{
    const int R = g.num_rows, NC = g.num_columns;
    const int* org = original_index + (size_t) s * (size_t) slots * (size_t) NC * (size_t) R;
    unsigned char* gr = is_ground + (size_t) s * (size_t) slots * (size_t) max_points;
    unsigned* det = detection + (size_t) s * (size_t) slots * (size_t) max_points;
    for (int row = lane_id(); row < R; row += 64)
    {
        const int ci = lc * R + row;
        if (scatter_cell_has_return(p, ci))
        {
            const unsigned seq = p.src[ci];
            const int frame = (int) (seq / (unsigned) NC), col = (int) (seq % (unsigned) NC);
            const int pt = org[((size_t) (frame % slots) * NC + col) * R + row];
            if (pt >= 0 && pt < max_points)
            {
                const size_t o = (size_t) (frame % slots) * (size_t) max_points + (size_t) pt;
                gr[o] = p.ground[ci] == CC_GP_GROUND ? 1 : 0;
                det[o] = cell_cluster_id(p, ci, (int) g.cells);
            }
        }
    }
}

// =====================================================================================================
// k_scatter_info / k_scatter_apply — the scatter for columns [from, from + grid) of ONE stream. grid = columns, block = 64. The caller names the
// columns, so the kernels test them: only a published column that has not been cleared, clear_done <= column < first_unpublished, holds what this
// reads (clearing is deferred by one call, so what a call published stays readable behind ring_start); anything else is "no point", like an
// empty column.
// =====================================================================================================
__global__ __launch_bounds__(64) void k_scatter_info(Geometry g, Planes P, const StreamState* __restrict__ states, int s, long long from,
                                                     const int* __restrict__ original_index, int slots, int* __restrict__ out_min,
                                                     int* __restrict__ out_max)
{
    const long long gc = from + blockIdx.x;
    const bool live = gc >= 0 && gc >= states[s].clear_done && gc < states[s].first_unpublished;
    scatter_column_info(g, stream_ptrs(P, g, s), s, (int) (gc % g.ring_cols), live, original_index, slots, out_min + blockIdx.x, out_max + blockIdx.x);
}

__global__ __launch_bounds__(64) void k_scatter_apply(Geometry g, Planes P, const StreamState* __restrict__ states, int s, long long from,
                                                      const int* __restrict__ original_index, int slots, unsigned char* __restrict__ is_ground,
                                                      unsigned* __restrict__ detection, long long max_points)
{
    const long long gc = from + blockIdx.x;
    if (gc < 0 || gc < states[s].clear_done || gc >= states[s].first_unpublished)
        return; // (not a published column that is still held)
    scatter_column_apply(g, stream_ptrs(P, g, s), s, (int) (gc % g.ring_cols), original_index, slots, is_ground, detection, max_points);
}

// =====================================================================================================
// k_replay_poke — cc_replay_eval_seek / cc_replay_eval_set_active in stream order (no synchronisation). One thread.
// =====================================================================================================
__global__ void k_replay_poke(ReplayState* __restrict__ state, int s, int seek, long long column, int prev, int set_active, int active)
{
    ReplayState st = state[s];
    if (seek)
    {
        st.cursor = column;
        st.prev = prev;
        st.error = 0;
        st.error_column = -1;
    }
    if (set_active)
        st.active = active;
    state[s] = st;
}

// =====================================================================================================
// k_replay_plan — per stream: the range this step walks, what was lost in front of it, the error that keeps the stream from walking.
// One thread per stream; the table goes to device memory and to pinned host memory (the host sizes the grids by the longest range).
// =====================================================================================================
__global__ __launch_bounds__(64) void k_replay_plan(Geometry g, const StreamState* __restrict__ states, const ReplayState* __restrict__ state,
                                                    cc_replay_stream* __restrict__ plan, cc_replay_stream* __restrict__ h_plan)
{
    const int s = (int) (blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= g.num_streams)
        return;
    const StreamState* st = &states[s];
    const ReplayState rs = state[s];
    const long long first = st->first_column, upper = st->first_unpublished;
    cc_replay_stream t;
    t.col_from = t.col_to = rs.cursor;
    t.lost_columns = 0;
    t.error_column = rs.error != 0 ? rs.error_column : -1;
    t.previous_frame = rs.prev;
    t.frames_evaluated = 0;
    t.error = rs.error != 0 ? rs.error : st->error;
    t.active = rs.active;
    if (t.error == 0 && rs.active != 0 && first >= 0 && upper >= 0)
    {
        const HeldRange r = held_range(first, st->clear_done, upper, rs.cursor, g.ring_cols);
        t.col_from = r.from;
        t.col_to = r.to;
        t.lost_columns = r.lost;
    }
    plan[s] = t;
    h_plan[s] = t;
    __threadfence_system();
}

// =====================================================================================================
// k_replay_info — scatter_column_info over the planned ranges of all streams. grid = (longest range, streams), block = 64: one wavefront per (column, stream), lanes = rows
// (two trips at 128 rows). out_min / out_max [s * stride + c] belong to column col_from + c.
// =====================================================================================================
__global__ __launch_bounds__(64) void k_replay_info(Geometry g, Planes P, const cc_replay_stream* __restrict__ plan, const int* __restrict__ original_index,
                                                    int slots, int* __restrict__ out_min, int* __restrict__ out_max, int stride)
{
    HeldColumn h;
    if (!held_column(g, P, plan, stride, &h))
        return;
    const size_t o = (size_t) h.s * stride + h.c;
    scatter_column_info(g, h.p, h.s, h.lc, true, original_index, slots, out_min + o, out_max + o);
}

// =====================================================================================================
// k_replay_walk — the column walk of addColumnAndEvaluateFrameIfCompleted over a stream's range, 64 columns per trip. grid = streams,
// block = 64 (lanes = columns). A segment ends with the first column whose largest frame is prev + 1 (kitti_demo.cpp:208-209): frame prev is
// complete, prev increments, the walk goes on behind that column with the new prev. A segment that holds a column whose smallest frame is
// < prev (:203-204) or whose largest frame is > prev + 1 (:205-206) is not applied: the walk stops in front of it with the error (the first of
// the two wins when a segment holds both, as the host walk tests them in that order). After max_done completed frames the walk stops behind
// the closing column and leaves the rest to the next step (the job list has that many places per stream). finish[s] != 0 (pinned host memory or
// null) completes frame prev as well and makes the stream inactive, unless the stream has an error.
// =====================================================================================================
__global__ __launch_bounds__(64) void k_replay_walk(const cc_replay_stream* __restrict__ plan, const ReplayState* __restrict__ state,
                                                    const int* __restrict__ in_min, const int* __restrict__ in_max, int stride, int max_done,
                                                    const unsigned char* __restrict__ finish, ReplayWalk* __restrict__ walk)
{
    const int s = (int) blockIdx.x, lane = lane_id();
    const cc_replay_stream pl = plan[s];
    const long long from = uniform_i64(pl.col_from);
    long long len = uniform_i64(pl.col_to) - from;
    len = len > stride ? stride : len;
    int prev = uniform_i32(state[s].prev);
    const int first_frame = prev;
    int n_done = 0, error = uniform_i32(pl.error);
    long long seg_start = 0;       // first column of the open segment, relative to `from`
    long long apply_to = len;
    bool seg_old = false, seg_far = false, stop = false;
    const int* mn_s = in_min + (size_t) s * stride;
    const int* mx_s = in_max + (size_t) s * stride;
    for (long long base = 0; base < len && !stop; base += 64)
    {
        const long long c = base + lane;
        const bool valid = c < len;
        const int mn = valid ? mn_s[c] : 0x7fffffff, mx = valid ? mx_s[c] : -1;
        const bool has = valid && mx >= 0;
        int start_lane = 0;
        while (start_lane < 64)
        {
            const unsigned long long behind = ~0ull << start_lane;
            const unsigned long long close = __ballot(has && mx == prev + 1) & behind;
            const unsigned long long old = __ballot(has && mn < prev) & behind;
            const unsigned long long far = __ballot(valid && mx > prev + 1) & behind;
            if (close == 0ull)
            {
                seg_old |= old != 0ull;
                seg_far |= far != 0ull;
                break; // (the segment goes on in the next trip)
            }
            const int L = __ffsll((unsigned long long) close) - 1;
            const unsigned long long upto = L == 63 ? ~0ull : ((1ull << (L + 1)) - 1ull);
            seg_old |= (old & upto) != 0ull;
            seg_far |= (far & upto) != 0ull;
            if (seg_old || seg_far)
            {
                stop = true;
                break;
            }
            n_done++;
            prev++;
            seg_start = base + L + 1;
            start_lane = L + 1;
            if (n_done >= max_done)
            {
                apply_to = seg_start;
                stop = true;
                break;
            }
        }
    }
    long long error_column = pl.error_column;
    if (error == 0 && (seg_old || seg_far))
    {
        error = seg_old ? CC_REPLAY_ERR_ALREADY_EVALUATED : CC_REPLAY_ERR_TOO_FAR_AHEAD;
        error_column = from + seg_start;
        apply_to = seg_start;
    }
    int active = pl.active;
    if (finish && finish[s] != 0 && error == 0 && active != 0)
    {
        n_done++; // "also evaluate final frame" (kitti_demo.cpp:417-419)
        prev++;
        active = 0;
    }
    if (lane == 0)
    {
        ReplayWalk w;
        w.apply_to = from + apply_to;
        w.error_column = error_column;
        w.first_frame = first_frame;
        w.n_done = n_done;
        w.new_prev = prev;
        w.new_active = active;
        w.error = error;
        w.pad = 0;
        walk[s] = w;
    }
}

// =====================================================================================================
// k_replay_scan — exclusive scan of the streams' completed frames: every (stream, frame) gets its place in the evaluation list (ordered by
// stream, then frame), the verdict on the caller's capacity, the finished table to pinned host memory, and — only when everything fits — the
// streams' new cursor, previous_frame, active flag and sticky error. grid = 1, block = TAKE_SCAN_THREADS.
// =====================================================================================================
__global__ __launch_bounds__(TAKE_SCAN_THREADS) void k_replay_scan(int num_streams, cc_replay_stream* __restrict__ plan, const ReplayWalk* __restrict__ walk,
                                                                   ReplayState* __restrict__ state, long long capacity, int job_capacity,
                                                                   ReplayJob* __restrict__ jobs, ReplayJob* __restrict__ h_jobs, ReplayCtl* __restrict__ ctl,
                                                                   cc_replay_stream* __restrict__ h_plan, ReplayCtl* __restrict__ h_ctl)
{
    __shared__ long long s_buf[TAKE_SCAN_THREADS];
    const int t = (int) threadIdx.x;
    long long b, e;
    run_of(t, num_streams, &b, &e);
    long long sum = 0;
    for (long long i = b; i < e; i++)
        sum += walk[i].n_done;
    long long total;
    long long off = take_block_scan(s_buf, sum, &total);
    const bool fits = total <= capacity && total <= job_capacity;
    for (int i = (int) b; i < e; i++)
    {
        const ReplayWalk w = walk[i];
        cc_replay_stream r = plan[i];
        r.col_to = w.apply_to;
        r.frames_evaluated = w.n_done;
        r.error = w.error;
        r.error_column = w.error_column;
        if (fits)
        {
            r.previous_frame = w.new_prev;
            r.active = w.new_active;
            for (int k = 0; k < w.n_done; k++)
            {
                ReplayJob j;
                j.stream = i;
                j.frame = w.first_frame + k;
                jobs[off + k] = j;
                h_jobs[off + k] = j;
            }
            ReplayState st = state[i];
            st.prev = w.new_prev;
            st.active = w.new_active;
            const bool raised = w.error == CC_REPLAY_ERR_ALREADY_EVALUATED || w.error == CC_REPLAY_ERR_TOO_FAR_AHEAD;
            if (raised || w.error == 0)
                st.cursor = w.apply_to; // (a stream with an engine error keeps its cursor)
            if (raised)
            {
                st.error = w.error;
                st.error_column = w.error_column;
            }
            state[i] = st;
        }
        off += w.n_done;
        plan[i] = r;
        h_plan[i] = r;
    }
    if (t == 0)
    {
        ReplayCtl c;
        c.total = total;
        c.capacity = capacity;
        c.fits = fits ? 1 : 0;
        c.pad = 0;
        *ctl = c;
        *h_ctl = c;
    }
    __threadfence_system();
}

// =====================================================================================================
// k_replay_apply — scatter_column_apply over the applied ranges [col_from, col_to) of all streams (col_to is the walk's apply-to column by
// now). Nothing is written unless every record fits. grid = (longest range, streams), block = 64.
// =====================================================================================================
__global__ __launch_bounds__(64) void k_replay_apply(Geometry g, Planes P, const cc_replay_stream* __restrict__ plan, const ReplayCtl* __restrict__ ctl,
                                                     const int* __restrict__ original_index, int slots, unsigned char* __restrict__ is_ground,
                                                     unsigned* __restrict__ detection, long long max_points)
{
    if (uniform_i32(ctl->fits) == 0)
        return; // (all or nothing)
    HeldColumn h;
    if (!held_column(g, P, plan, 0x7fffffff, &h)) // (no per-stream array)
        return;
    scatter_column_apply(g, h.p, h.s, h.lc, original_index, slots, is_ground, detection, max_points);
}

// =====================================================================================================
// k_replay_eval — the label compare of the round's frames: evaluation lane blockIdx.y takes job first_job + blockIdx.y on its own counters and
// its own table (ccev::eval_point: k_eval's body). grid = (blocks over the largest n_points of the round, frames of the round), block = 256.
// The first thread of the launch also empties the pair counter k_replay_compact counts with (nobody else touches it in this launch).
// =====================================================================================================
__global__ __launch_bounds__(256) void k_replay_eval(const ReplayJob* __restrict__ jobs, int first_job, int slots, long long max_points,
                                                     const long long* __restrict__ n_points, const uint16_t* __restrict__ semantic,
                                                     const uint32_t* __restrict__ euclid, const unsigned char* __restrict__ is_ground,
                                                     const unsigned* __restrict__ detection, unsigned long long* __restrict__ counts,
                                                     unsigned long long* __restrict__ keys, unsigned* __restrict__ vals, unsigned table,
                                                     unsigned long long* __restrict__ n_pairs)
{
    const int lane = (int) blockIdx.y;
    if (blockIdx.x == 0 && lane == 0 && threadIdx.x == 0)
        *n_pairs = 0ull;
    const ReplayJob j = jobs[first_job + lane];
    const size_t fs = (size_t) j.stream * (size_t) slots + (size_t) replay_slot(j.frame, slots);
    long long n = n_points[fs];
    n = n > max_points ? max_points : n;
    if ((long long) blockIdx.x * 256 >= n)
        return; // (whole block: the ballots of eval_point stay complete)
    const size_t o = fs * (size_t) max_points;
    ccev::eval_point((long long) blockIdx.x * 256 + threadIdx.x, n, semantic + o, euclid + o, is_ground + o, detection + o,
                     counts + (size_t) lane * REPLAY_COUNTS, keys + (size_t) lane * table, vals + (size_t) lane * table, table - 1u);
}

// =====================================================================================================
// k_replay_compact — the distinct pairs of the round's lanes as (key, count, lane) behind one counter, straight into pinned host memory, and
// the lanes' five counters next to them. Every slot and counter is restored to empty as it is read: the next round (and the next step) finds
// clean tables without a memset. grid = (table / 256, frames of the round), block = 256.
// =====================================================================================================
__global__ __launch_bounds__(256) void k_replay_compact(unsigned table, unsigned long long* __restrict__ keys, unsigned* __restrict__ vals,
                                                        unsigned long long* __restrict__ counts, unsigned long long* __restrict__ n_pairs,
                                                        unsigned long long pair_capacity, ReplayPair* __restrict__ h_pairs,
                                                        unsigned long long* __restrict__ h_counts)
{
    const int lane = (int) blockIdx.y;
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x < REPLAY_COUNTS)
    {
        h_counts[(size_t) lane * REPLAY_COUNTS + threadIdx.x] = counts[(size_t) lane * REPLAY_COUNTS + threadIdx.x];
        counts[(size_t) lane * REPLAY_COUNTS + threadIdx.x] = 0ull;
    }
    if (i >= table)
        return;
    const size_t at = (size_t) lane * table + i;
    const unsigned long long key = keys[at];
    if (key != ccev::EMPTY)
    {
        const unsigned long long o = atomicAdd(n_pairs, 1ull);
        if (o < pair_capacity) // (always: a lane has at most max_points distinct pairs)
        {
            ReplayPair pr;
            pr.key = key;
            pr.count = vals[at];
            pr.lane = (unsigned) lane;
            h_pairs[o] = pr;
        }
        keys[at] = ccev::EMPTY;
        vals[at] = 0u;
    }
}
