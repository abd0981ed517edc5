// cc_launch.h — the batch launch path of the engine: what goes onto which HIP stream, stage by stage, and launch_batch, which orders the stages of
// one pass. Host code only. Not a header of its own: cc_engine.hip includes it once, inside its anonymous namespace, behind the definitions the
// stages use (cc_engine, CC_HIP_CHECK, cc_buffers.h for ensure_ego, TimingMark, launch_prep, flush_deferred, the lazy-gate predicates, k_begin_batch,
// k_gate_out, finish_batch).
// ---- rows per lane -------------------------------------------------------------------------------------------------------------------------
// The kernels that walk a column's rows are templates on the rows one lane holds (1: up to 64 rows, 2: up to 128). Every launch of one has ONE
// argument list: CC_LAUNCH_RPL picks the instantiation from `rpl_`; CC_LAUNCH_RPL_MIRROR picks the <RPL, MIRROR> pair of the window scans
// from `rpl_` and Geometry::mirror_fields; CC_LAUNCH_RPL_T appends further template arguments (CC_TARGS(, false, true): k<RPL, false, true>).
#define CC_TARGS(...) __VA_ARGS__
#define CC_LAUNCH_RPL_T(kern_, targs_, rpl_, grid_, block_, lds_, st_, ...)               \
    do                                                                                     \
    {                                                                                      \
        if ((rpl_) == 1)                                                                   \
            hipLaunchKernelGGL((kern_<1 targs_>), grid_, block_, lds_, st_, __VA_ARGS__); \
        else                                                                               \
            hipLaunchKernelGGL((kern_<2 targs_>), grid_, block_, lds_, st_, __VA_ARGS__); \
    } while (0)
#define CC_LAUNCH_RPL(kern_, rpl_, ...) CC_LAUNCH_RPL_T(kern_, , rpl_, __VA_ARGS__)
#define CC_LAUNCH_RPL_MIRROR(kern_, rpl_, mirror_, ...)                   \
    do                                                                    \
    {                                                                     \
        if (mirror_)                                                      \
            CC_LAUNCH_RPL_T(kern_, CC_TARGS(, true), rpl_, __VA_ARGS__);  \
        else                                                              \
            CC_LAUNCH_RPL_T(kern_, CC_TARGS(, false), rpl_, __VA_ARGS__); \
    } while (0)

// ---- one pass over a batch -----------------------------------------------------------------------------------------------------------------
// What a pass is. launch_batch fills it once, at its top; the stages below only read it. The closures that run later (the deferred tail, the lazy
// gate) hold a copy: a pass carries its own cur_ntotal / cur_f0 / prep_buf because by the time they run the engine's fields are the NEXT batch's.
struct BatchPass
{
    hipStream_t si, sb, sc, sa, sp; // insertion | table + segmentation | window scan | association | preparation (all equal when not pipelined)
    int slot, first_stream, count;
    int64_t n;
    const float* d_xyz; // the caller's buffers
    const uint8_t* d_int;
    const double* d_pose;
    bool first_pass, prep_done;
    int rpl;                      // rows per lane
    long long cur_ntotal, cur_f0; // this batch is firings [cur_f0, cur_f0 + n) of buffers holding cur_ntotal per stream
    int prep_buf;                 // the staging buffer its points were (or will be) prepared into
    Planes Pt;                    // k_table -> k_seg_scan scratch of this batch-descriptor slot (up to BATCH_SLOTS batches are in flight)
    double* d_ego;                // per-firing ego transforms of this batch (one buffer per descriptor slot: up to three batches are in flight)
    int *gate_left, *gate_h_left; // (one pair of counters per batch descriptor slot: the lazy gate reads a batch's pair while the next batch runs)
    bool par, gate, gate2, may_defer, lazy, fuse;
    uint64_t rel_seq;             // the call this batch is the end of (0: a continuation pass, a sub-batch that is not its call's last, a call on the host path)
    bool mark;                    // this pass records its TimingMark events
    hipEvent_t ev[NEV];
};

// what is known about a batch's insertion when the chains behind it are launched (the lazy gate learns it later than the plain one)
struct TailArgs
{
    bool fallbacks;   // some stream's batch was not taken completely by k_insert_par (/ k_insert_multi): k_prep and k_insert2 have work
    bool need_segpre; // some stream's batch is not closed as fused: k_table / k_seg_pre have work
    bool pre_done;    // the insertion stream's part of the tail (ev1, ev2, the early-stop counter, ev_ins) was enqueued in front of the gate
    bool hp_gated;    // CC_HOST_PROF: the host waited at a gate, until hp_t1
    std::chrono::steady_clock::time_point hp_t1;
};

#define CC_MARK(which_, st_) \
    if (bp.mark)             \
        CC_HIP_CHECK(e, hipEventRecord(bp.ev[which_], st_));

// the per-firing ego records of a batch (they only depend on the caller's poses and the robot transform): in front of the fused insertion on the
// insertion chain, else in front of k_seg_pre / k_seg_small on the segmentation chain
static void launch_ego(cc_engine* e, const BatchPass& bp, hipStream_t st)
{
    hipLaunchKernelGGL(cck::k_ego, dim3((unsigned) ((bp.n + 255) / 256), (unsigned) bp.count), dim3(256), 0, st, (const StreamState*) e->d_states, bp.first_stream,
                       e->cfg, bp.d_pose, (long long) bp.n, bp.cur_ntotal, bp.cur_f0, bp.d_ego);
}

// ---- fused insertion: k_ego, k_insert_par (+ k_insert_par_fin), k_gate_out on the insertion chain --------------------------------------------
// prev_left: the counters of the previous batch's insertion when this one is enqueued before the host has read them (lazy gate)
// lazy: this batch's own counters will be read by the next call — what the held-back chains need of the insertion stream (the early-stop
// counter, the event the segmentation chain waits for) and the event the NEXT call waits for follow the insertion
static int enqueue_fused_insertion(cc_engine* e, const BatchPass& bp, const int* prev_left, const bool lazy)
{
    const Geometry& g = e->g;
    const hipStream_t si = bp.si;
    const int count = bp.count;
    const double* ego_in = bp.fuse ? (const double*) bp.d_ego : (const double*) nullptr;
    int* left = bp.gate ? bp.gate_left : (int*) nullptr;
    const bool gate_zeroed = bp.gate && bp.first_pass && si != bp.sb && !use_small_front(e, count, bp.n, true); // (submit's k_begin_batch zeroed the counters)
    if (bp.fuse)
    {
        // the fused insertion needs the per-firing ego records (they only depend on the caller's poses and the robot transform, which the
        // host writes between batches): k_ego runs in front of it on the insertion chain. (On the preparation stream, beside the previous
        // batch's insertion, it measured slower: the cross-stream event costs more than the kernel's ~10 us on the chain.) The records'
        // buffer belongs to the batch-descriptor slot: its last readers (segmentation chain of four batches ago) are in front of that
        // slot's publishing event.
        launch_ego(e, bp, si);
    }
    if (bp.gate && !gate_zeroed)
        CC_HIP_CHECK(e, hipMemsetAsync(left, 0, 2 * sizeof(int), si));
    // few streams: the GPU is not full and the insertion chain is what a step waits for -> twice the wavefronts per block, and the firings of a
    // stream dealt to several blocks (k_insert_par_fin then finishes the stream's state)
    if (count <= e->insert_wide_max_streams)
    {
        // (round 4: with the segmentation fused in, a block of 8 wavefronts needs ~1.1 ms per 2200 firings by itself: up to 160 streams the
        // GPU has room for twice the wavefronts — 128 streams 11.3 -> 15.0 G points/s — above that it is full and they only get in each other's way)
        // (blocks per stream, same-box alternations over 40 steps: 4 up to 40 streams; 3 up to 64 — 48 streams 12.3 -> 12.9 - 13.0 G points/s and 64 streams
        // 14.0 - 14.2 -> 14.4 - 14.6 against 2 blocks, 4 blocks at 64 streams - 5 %; 2 up to 96 — at 80 streams 3 blocks are 5 - 8 % slower than 2)
        // A block of 16 wavefronts wants a compute unit it does not share with a block of k_assocb (one per stream, 16 wavefronts too): blocks x streams + streams <= 256
        // is where more blocks stop paying — 32 streams: 4 / 6 / 7 / 8 blocks 11.3 / 11.7 - 12.0 / 11.6 - 12.0 / 9.7 G points/s; 24 and 16 streams: 8 blocks + 1 .. + 3 % against 4;
        // 40 streams: 5 blocks - 3 .. - 5 % against 4 (the rule is not exact: measured points decide)
        const int nb = e->insert_split_blocks > 0 ? e->insert_split_blocks
                                                  : (count <= 24 ? 8 : (count <= 32 ? 6 : (count <= 40 ? 4 : (count <= 64 ? 3 : (count <= 96 ? 2 : 1)))));
        hipLaunchKernelGGL((cck::k_insert_par<1, 2 * cck::IP_WAVES>), dim3(count, nb), dim3(128 * cck::IP_WAVES), 0, si, g, e->cfg, bp.Pt, e->d_states,
                           bp.first_stream, bp.d_xyz, bp.d_int, bp.d_pose, (long long) bp.n, bp.cur_ntotal, bp.cur_f0, bp.slot, left, ego_in, prev_left);
        if (nb > 1)
            hipLaunchKernelGGL(cck::k_insert_par_fin<1>, dim3(count), dim3(256), 0, si, g, bp.Pt, e->d_states, bp.first_stream, bp.d_xyz, (long long) bp.n,
                               bp.cur_ntotal, bp.cur_f0, bp.slot, left, bp.fuse ? 1 : 0, prev_left);
    }
    else
        hipLaunchKernelGGL((cck::k_insert_par<1, cck::IP_WAVES>), dim3(count), dim3(64 * cck::IP_WAVES), 0, si, g, e->cfg, bp.Pt, e->d_states,
                           bp.first_stream, bp.d_xyz, bp.d_int, bp.d_pose, (long long) bp.n, bp.cur_ntotal, bp.cur_f0, bp.slot, left, ego_in, prev_left);
    if (bp.gate)
    {
        // (the counter of k_assocb's stops rides along: as of whatever the association chain has finished by now — it only steers a heuristic;
        // with the lazy gate also the early-stop counter the held-back chains would have copied)
        hipLaunchKernelGGL(k_gate_out, dim3(1), dim3(64), 0, si, (const int*) left, (const int*) e->d_bail_count, (const int*) e->d_remaining, bp.gate_h_left,
                           e->h_bail_count, lazy ? e->h_remaining : (int*) nullptr);
    }
    if (lazy)
    {
        CC_HIP_CHECK(e, hipEventRecord(e->ev_ins[bp.slot], si));
        CC_HIP_CHECK(e, hipEventRecord(e->ev_gate[bp.slot], si));
    }
    return CC_OK;
}

// ---- host gate: the host waits for the insertion chain and then reads the counters the kernels in front left for it ---------------------------
// (both gates: behind k_insert_par, whose k_gate_out wrote them into pinned memory, and behind k_insert_multi<2>, whose copies were enqueued)
static int wait_host_gate(cc_engine* e, const BatchPass& bp, const std::chrono::steady_clock::time_point hp_t0, TailArgs& ta)
{
    const auto hp1 = std::chrono::steady_clock::now();
    CC_HIP_CHECK(e, hipStreamSynchronize(bp.si));
    ta.hp_t1 = std::chrono::steady_clock::now();
    if (e->host_prof)
    {
        e->hp_pre += std::chrono::duration<double>(hp1 - hp_t0).count();
        e->hp_gate += std::chrono::duration<double>(ta.hp_t1 - hp1).count();
        ta.hp_gated = true;
    }
    return CC_OK;
}

// ---- insertion fall-backs -------------------------------------------------------------------------------------------------------------------
// multi-column firings (per-laser azimuth offsets) and whatever single-column head k_insert_par did not take: block-parallel as well,
// with the per-row collision rule checked instead of assumed (option "parallel_insert" = 2 restricts this to the first kernel)
// (above 64 rows it is the first insertion kernel, and the gate is here: k_prep and k_insert2<2> — 96 KB of LDS per block — stood 1.3 ms per batch in
// the insertion chain of 256 VLS-128-shaped streams, the chain the host waits for, to find nothing to do)
static int enqueue_insert_multi(cc_engine* e, const BatchPass& bp, const std::chrono::steady_clock::time_point hp_t0, TailArgs& ta)
{
    const hipStream_t si = bp.si;
    if (bp.gate2)
        CC_HIP_CHECK(e, hipMemsetAsync(e->d_par_left, 0, sizeof(int), si));
    int* left2 = bp.gate2 ? e->d_par_left : (int*) nullptr; // (null with one row per lane: only k_insert_multi<2> counts for a gate)
    CC_LAUNCH_RPL(cck::k_insert_multi, bp.rpl, dim3(bp.count), dim3(64 * cck::IM_WAVES), 0, si, e->g, e->cfg, e->P, e->d_states, bp.first_stream, bp.d_xyz,
                  bp.d_int, bp.d_pose, (long long) bp.n, bp.cur_ntotal, bp.cur_f0, bp.slot, left2);
    if (bp.gate2)
    {
        CC_HIP_CHECK(e, hipMemcpyAsync(e->h_par_left, e->d_par_left, sizeof(int), hipMemcpyDeviceToHost, si));
        if (e->h_bail_count)
            CC_HIP_CHECK(e, hipMemcpyAsync(e->h_bail_count, e->d_bail_count, 3 * sizeof(int), hipMemcpyDeviceToHost, si));
        int rcw = wait_host_gate(e, bp, hp_t0, ta);
        if (rcw)
            return rcw;
        ta.fallbacks = *e->h_par_left != 0;
    }
    return CC_OK;
}

// k_prep + k_insert2 for what the block-parallel kernels left, and the end of the insertion chain's own part: ev1, ev2, the early-stop counter
static int enqueue_insert_serial(cc_engine* e, const BatchPass& bp, const TailArgs& ta)
{
    const hipStream_t si = bp.si, sp = bp.sp;
    if (bp.first_pass && !bp.prep_done && ta.fallbacks) // relaunch passes of the same batch reuse the staged points; a pipelined caller prepared ahead
    {
        int rcp = launch_prep(e, bp.count, bp.n, bp.d_xyz, bp.d_pose, bp.prep_buf, sp, bp.cur_ntotal, bp.cur_f0, bp.par, bp.first_stream);
        if (rcp)
            return rcp;
    }
    if (!ta.pre_done)
        CC_MARK(EV_PREP, sp); // ev1: prep (with k_insert_par in front of it when that is on)
    if (sp != si)
    {
        CC_HIP_CHECK(e, hipEventRecord(e->ev_prep[bp.slot], sp));
        CC_HIP_CHECK(e, hipStreamWaitEvent(si, e->ev_prep[bp.slot], 0));
    }
    if (ta.fallbacks)
    {
        const Planes Pins = planes_with_prep(e, bp.prep_buf);
        CC_LAUNCH_RPL(cck::k_insert2, bp.rpl, dim3(bp.count), dim3(128), cck::insert2_lds_bytes(e->g.num_rows), si, e->g, e->cfg, Pins, e->d_states,
                      bp.first_stream, bp.slot, bp.d_int, (long long) bp.n, e->d_remaining, bp.cur_ntotal, bp.cur_f0);
    }
    if (!ta.pre_done)
        CC_MARK(EV_INSERT, si); // ev2: insert
    if (!ta.pre_done && !e->capture_mirror.state) // (a small call's graph gets the counter through k_publish's mirror)
        CC_HIP_CHECK(e, hipMemcpyAsync(e->h_remaining, e->d_remaining, sizeof(int), hipMemcpyDeviceToHost, si));
    return CC_OK;
}

// ---- table + segmentation chain: k_table, k_ego, k_seg_pre, k_seg_small / k_seg_scan ------------------------------------------------------------
static int launch_segmentation(cc_engine* e, const BatchPass& bp, const TailArgs& ta)
{
    const Geometry& g = e->g;
    const hipStream_t si = bp.si, sb = bp.sb, sc = bp.sc;
    // k_table only needs what the insertion of this batch wrote. It is a latency-bound kernel (8 wavefronts per stream) that takes 0.8 ms
    // when it shares the GPU with the throughput kernels — on the segmentation chain, which is the longest of the three, that is a
    // third of the chain; at the end of the insertion chain, which has slack, it costs nothing.
    // calls of a few firings (the per-column latency path): ONE wavefront per stream segments the call's columns, rows as lanes (k_seg_small)
    const bool seg_small = !bp.par && bp.rpl == 1 && bp.first_pass && bp.n <= e->seg_small_max;
    const bool need_segpre = ta.need_segpre && !seg_small;
    // (with the fused front half k_insert_par reads and writes the running table `curtab` on the insertion chain: k_table of a batch that is not
    // fused has to run on that chain too — elsewhere nothing would order it against the next batch's insertion)
    const bool table_early = si != sb;
    if (table_early && need_segpre)
        CC_LAUNCH_RPL(cck::k_table, bp.rpl, dim3(bp.count), dim3(64 * cck::TABLE_WAVES), 0, si, g, bp.Pt, e->d_states, bp.first_stream, bp.slot);
    if (si != sb)
    {
        if (!ta.pre_done)
            CC_HIP_CHECK(e, hipEventRecord(e->ev_ins[bp.slot], si));
        CC_HIP_CHECK(e, hipStreamWaitEvent(sb, e->ev_ins[bp.slot], 0));
    }
    CC_MARK(EV_CHAIN2, sb); // ev3: start of the second chain
    if (!table_early && need_segpre)
        CC_LAUNCH_RPL(cck::k_table, bp.rpl, dim3(bp.count), dim3(64 * cck::TABLE_WAVES), 0, sb, g, bp.Pt, e->d_states, bp.first_stream, bp.slot);
    if (need_segpre)
    {
        if (!bp.fuse) // (the fused insertion had k_ego in front of it)
            launch_ego(e, bp, sb);
        CC_LAUNCH_RPL(cck::k_seg_pre, bp.rpl, dim3((unsigned) bp.count, cck::SEGPRE_BLOCKS), dim3(64), 0, sb, g, e->cfg, bp.Pt, e->d_states, bp.first_stream,
                      bp.slot, bp.d_pose, bp.cur_ntotal, bp.cur_f0, (const double*) bp.d_ego, (long long) bp.n);
    }
    if (seg_small)
    {
        launch_ego(e, bp, sb);
        hipLaunchKernelGGL(cck::k_seg_small, dim3((unsigned) bp.count), dim3(64), 0, sb, g, e->cfg, e->P, e->d_states, bp.first_stream, bp.slot, bp.d_pose,
                           bp.cur_ntotal, bp.cur_f0, (const double*) bp.d_ego, (long long) bp.n);
    }
    else
    {
        // an upper bound of the columns one pass can emit: the in-kernel limit plus half a rotation of one firing
        const long long max_cols = std::min<long long>((long long) g.limit_columns + g.num_columns, (long long) g.ring_cols);
        // grids are (streams, blocks): the stream index is the fast dimension so that one stream's blocks share an XCD (and its L2)
        const dim3 seg_grid((unsigned) bp.count, (unsigned) ((max_cols + 63) / 64));
        hipLaunchKernelGGL(cck::k_seg_scan, seg_grid, dim3(64), cck::seg_scan_lds_bytes(g.num_rows), sb, g, e->cfg, bp.Pt, e->d_states, bp.first_stream,
                           bp.slot); // (Pt: this slot's table carries)
    }
    if (sc != sb)
    {
        CC_HIP_CHECK(e, hipEventRecord(e->ev_segscan[bp.slot], sb));
        CC_HIP_CHECK(e, hipStreamWaitEvent(sc, e->ev_segscan[bp.slot], 0));
    }
    CC_MARK(EV_SEGMENT, sc); // ev4: table + segment (start of the window scan)
    return CC_OK;
}

// ---- what the association chain of this batch will be (decided in front of the window scan, which writes Planes::sc_fin only for the serial kernels) ----
struct AssocPlan
{
    bool batch_assoc;    // k_assocb in front of the serial kernels
    int rounds;          // (k_assocb, k_assoc3) pairs
    int blocks;          // blocks of every k_assoc3 launch: a few that sweep over all streams, or one per stream
    bool lwave;          // k_assoc3 with its links wavefront
    int scan_stores_fin; // Geometry::scan_stores_fin of this batch's window scan and serial association kernels
};

// (reads *e->h_bail_count as of this moment — whatever the gate or an earlier batch's association chain copied last — and moves the engine's
// chronic-stop and cooldown counters on by one batch)
static AssocPlan plan_association(cc_engine* e, const BatchPass& bp, const bool small_front)
{
    const int count = bp.count;
    bool batch_assoc = e->assoc_batch && e->cfg.cluster_point_trees_every_nth_column == 1;
    // Streams on which k_assocb keeps stopping (vegetation: more trees born per group than it has lanes for) cost a batch more with it than
    // without: every stop is a (batch-parallel, serial) round, and a launch lasts as long as its slowest stream — the one that went serial.
    // While at least a quarter of a launch's streams stop per batch the serial kernels run alone; every ninth batch tries again.
    if (batch_assoc && e->assoc_rounds == 0 && e->h_bail_count && !e->capturing && count >= 8)
    {
        const int seen_now = *e->h_bail_count;
        if (e->chronic_skip > 0)
        {
            e->chronic_skip--;
            e->bail_seen = seen_now;
            batch_assoc = false;
            // (the batches that try again must not meet the two sweeping blocks the serial kernel runs as behind an idle k_assocb)
            if (e->chronic_skip == 0)
                e->bail_cooldown = e->bail_cooldown_batches > 2 ? e->bail_cooldown_batches : 2;
        }
        else if ((seen_now - e->chronic_seen) * 4 >= count && e->chronic_probe)
            e->chronic_skip = 8;
        e->chronic_probe = batch_assoc; // (the counter read behind the NEXT batch tells what this one did)
        e->chronic_seen = seen_now;
    }
    int adaptive_rounds = 1;
    if (e->assoc_rounds == 0 && e->h_bail_count && !e->capturing)
    {
        const int seen = *e->h_bail_count; // (as of some earlier batch: a heuristic, not a condition of correctness)
        if (seen != e->bail_seen)
        {
            e->bail_seen = seen;
            e->bail_cooldown = e->bail_cooldown_batches;
        }
        if (e->bail_cooldown > 0)
        {
            e->bail_cooldown--;
            adaptive_rounds = 3;
        }
    }
    AssocPlan plan{batch_assoc, batch_assoc ? (e->assoc_rounds > 0 ? e->assoc_rounds : adaptive_rounds) : 1, count, false, 0};
    // behind k_assocb the serial kernel is a safety net that finds nothing to do: a few blocks sweep over all streams instead of one block
    // per stream waiting for 45 KB of LDS on a busy CU. One block per stream when it is what associates, or while k_assocb has had to stop
    // lately (adaptive_rounds > 1), or when the caller pinned the number of rounds
    const bool idle_net = batch_assoc && e->assoc_rounds == 0 && adaptive_rounds == 1;
    if (idle_net && !e->capturing && e->assoc_sweep_blocks < count)
        plan.blocks = e->assoc_sweep_blocks;
    // with or without the links wave (cc_assoc3.h: A3_THREADS): by default (assoc_waves = 0) with it while the streams are few
    // enough for the association chain to be what the step waits for
    plan.lwave = e->assoc_waves == 4 || (e->assoc_waves_auto && count <= CC_LWAVE_MAX_STREAMS);
    // The serial kernels read a point's finished_at contribution from Planes::sc_fin or recompute it (cc_k_base.h: cell_fin_of). Behind the
    // batch-parallel kernel they find nothing to do, and the scan saves the 8 bytes per cell; where they are expected to associate (the
    // batch-parallel kernel off, pinned rounds, stops lately) the scan stores them. A small call's front kernel has scanned with the engine's
    // geometry (never stored).
    plan.scan_stores_fin = (!small_front && !idle_net) ? 1 : 0;
    if (e->scan_store_fin >= 0 && !small_front)
        plan.scan_stores_fin = e->scan_store_fin;
    return plan;
}

// ---- packed (k_scan2) or lock-step (k_scan) window scan, and the long scans apart or not ---------------------------------------------------------
struct ScanChoice
{
    bool packed, split;
};

// (65 - 128 rows: packed by default. The lock-step form with two rows per lane — scan_packed = 0 — shortens the scan's own launch, 3.0 -> 2.35 ms at
// 256 x S128, but needs more vector instructions, and the step is bound by those: 11.7 -> 11.4 G points/s same-box)
// (64 rows, end of round 4: with the insertion's uniform work on the scalar unit the step follows the vector-instruction count, and the packed
// scan issues 0.65 x those of the lock-step one: + 3 % at 256 streams (same-box, 3 alternations: 16.22 -> 16.72 G points/s), - 1 ... - 2 % at
// 32 - 128 streams where the GPU has room and the lock-step scan's shorter launch counts)
// (counts a batch in the automatic mode's books: split_on, split_cols_seen, split_rec_seen, split_probe)
static ScanChoice choose_scan(cc_engine* e, const BatchPass& bp)
{
    const int rpl = bp.rpl, count = bp.count;
    // the long scans apart? scan_split 1: always (with the packed scan); 2 (default): while they are a large part of the scan's work. The
    // visits k_scan2_long makes per column (of 64 rows) say so: vegetation ~150, the 128-row bench scene ~15, the street scene ~4. Where they
    // are few the split costs chain time (two more launches whose blocks wait for wave slots, the longest single scan standing alone: street
    // scene - 8 % at 256 streams, the 128-row scene - 2 %), on vegetation it is + 60 .. + 70 %. Every 32nd batch is scanned packed and with
    // the split, which counts; the batches counted since the last look decide (on above 40 visits per column, off again below 20).
    // On vegetation the packed scan with the split also beats the lock-step scan from 48 streams per launch (64 streams + 14 %, 128 + 38 %;
    // 32 streams - 4 %), where the street scene wants the lock-step one up to 192.
    const bool packed_default = e->scan_packed == 1 || (e->scan_packed < 0 && (rpl > 1 || count > 192));
    if (e->g.mirror_fields || e->scan_split == 0)
        return {packed_default, false};
    if (e->scan_split == 1 || !e->h_bail_count || e->capturing)
        return {packed_default, packed_default && e->scan_split == 1};
    const unsigned vis = (unsigned) e->h_bail_count[1], cols = (unsigned) e->h_bail_count[2];
    const unsigned dc = cols - e->split_cols_seen, dv = vis - e->split_rec_seen;
    if (dc >= 1024u)
    {
        const double rate = (double) dv / ((double) dc * (double) rpl); // (per column of 64 rows)
        e->split_on = e->split_on ? rate > 20.0 : rate > 40.0;
        e->split_cols_seen = cols, e->split_rec_seen = vis;
    }
    const bool probe = (e->split_probe++ & 31u) == 0u;
    const bool promote = !packed_default && e->scan_packed < 0 && rpl == 1 && count >= 48; // (launches the lock-step scan would take)
    const bool split = (e->split_on || probe) && (packed_default || promote);
    return {packed_default || (promote && split), split};
}

// ---- window-scan chain. `gs`: the engine's geometry with this batch's scan_stores_fin; the kernels of the long scans take the engine's own ----
static int launch_scan(cc_engine* e, const BatchPass& bp, const ScanChoice scan, const Geometry& gs)
{
    const Geometry& g = e->g;
    const hipStream_t sc = bp.sc;
    const dim3 scan_grid((unsigned) bp.count, cck::SCAN_BLOCKS);
    if (scan.packed && scan.split)
    {
        // long scans apart (cc_k_scan.h): the packed scan hands points that are still scanning after SCAN_CAP visits to k_scan2_long, which
        // keeps every lane busy with one of them; k_scan2_epi finishes the columns that had such a point
        const dim3 long_grid((unsigned) bp.count, cck::SCAN_LONG_BLOCKS), epi_grid((unsigned) bp.count, cck::SCAN_EPI_BLOCKS);
        CC_LAUNCH_RPL_T(cck::k_scan2, CC_TARGS(, false, true), bp.rpl, scan_grid, dim3(64), 0, sc, gs, e->cfg, e->P, e->d_states, bp.first_stream, bp.slot);
        CC_LAUNCH_RPL(cck::k_scan2_long, bp.rpl, long_grid, dim3(64), 0, sc, g, e->cfg, e->P, e->d_states, bp.first_stream, bp.slot, e->d_bail_count);
        CC_LAUNCH_RPL(cck::k_scan2_epi, bp.rpl, epi_grid, dim3(64), 0, sc, g, e->cfg, e->P, e->d_states, bp.first_stream, bp.slot, e->d_bail_count);
    }
    else if (scan.packed)
        CC_LAUNCH_RPL_MIRROR(cck::k_scan2, bp.rpl, g.mirror_fields, scan_grid, dim3(64), 0, sc, gs, e->cfg, e->P, e->d_states, bp.first_stream, bp.slot);
    else
        CC_LAUNCH_RPL_MIRROR(cck::k_scan, bp.rpl, g.mirror_fields, scan_grid, dim3(64), 0, sc, gs, e->cfg, e->P, e->d_states, bp.first_stream, bp.slot);
    CC_MARK(EV_SCAN, sc); // ev5: scan
    if (sc != bp.sa)
    {
        CC_HIP_CHECK(e, hipEventRecord(e->ev_seg[bp.slot], sc));
        CC_HIP_CHECK(e, hipStreamWaitEvent(bp.sa, e->ev_seg[bp.slot], 0));
    }
    return CC_OK;
}

// ---- association chain -------------------------------------------------------------------------------------------------------------------------
// batch-parallel association in front of the serial kernels: it takes every group of columns in which nothing can differ from the
// reference's sequential semantics (cc_assocb.h) and stops in front of the first group that might. With k_assoc3 behind it the pair runs
// assoc_rounds times: a LIMITED launch of the serial kernel takes that one group, the batch-parallel kernel continues behind it; the last
// serial launch takes whatever is left of the batch.
static void launch_assocb(cc_engine* e, const BatchPass& bp)
{
    CC_LAUNCH_RPL(cck::k_assocb, bp.rpl, dim3(bp.count), dim3(cck::AB_THREADS), 0, bp.sa, e->g, e->cfg, e->P, e->d_states, bp.first_stream, bp.slot,
                  e->d_bail_count);
}

static int launch_association(cc_engine* e, const BatchPass& bp, const AssocPlan& plan, const Geometry& gs)
{
    const hipStream_t sa = bp.sa;
    const int count = bp.count;
    CC_MARK(EV_CHAIN3, sa); // ev6: start of the third chain
    bool marked7 = false;
    bool global_done = false; // k_associate's work was done inside the last k_assoc3 launch
    // k_assoc3 walks the finished-cluster checks of several columns at once and assumes one check per column
    if (e->assoc_waves >= 2 && e->cfg.cluster_point_trees_every_nth_column == 1)
    {
        const dim3 block(plan.lwave ? cck::A3_THREADS : 192);
        for (int r = 0; r < plan.rounds; r++)
        {
            if (plan.batch_assoc)
            {
                launch_assocb(e, bp);
                if (r == 0)
                {
                    CC_MARK(EV_ASSOC_LDS, sa); // ev7: the batch-parallel kernel alone ("assoc_lds_ms"); the serial kernels behind it count as "assoc_global_ms"
                    marked7 = true;
                }
            }
            const int limited = r + 1 < plan.rounds ? 1 : 0;
            CC_LAUNCH_RPL(cck::k_assoc3, bp.rpl, dim3(plan.blocks), block, 0, sa, gs, e->cfg, e->P, e->d_states, bp.first_stream, bp.slot, limited, count, 1);
            global_done = limited == 0; // (the last launch of k_assoc3 takes the streams that continue in global memory with it)
        }
    }
    else
    {
        if (plan.batch_assoc)
        {
            launch_assocb(e, bp);
            CC_MARK(EV_ASSOC_LDS, sa);
            marked7 = true;
        }
        CC_LAUNCH_RPL(cck::k_assoc_lds, bp.rpl, dim3(count), dim3(64), 0, sa, gs, e->cfg, e->P, e->d_states, bp.first_stream, bp.slot);
    }
    if (!marked7)
        CC_MARK(EV_ASSOC_LDS, sa); // ev7: assoc_lds (without the batch-parallel kernel: the serial LDS kernel)
    // streams whose unfinished trees do not fit the LDS pool (or exotic window configs) continue in global memory
    if (!global_done)
        CC_LAUNCH_RPL(cck::k_associate, bp.rpl, dim3(count), dim3(64), 0, sa, e->g, e->cfg, e->P, e->d_states, bp.first_stream, bp.slot);
    CC_MARK(EV_ASSOC_GLOBAL, sa); // ev8: assoc_global
    return CC_OK;
}

// ---- publish, and the events that free the batch-descriptor slot and release the caller's buffers -----------------------------------------------
// (`with_publish` false: a small call's k_small_tail has written the ids and the mirror)
static int publish_and_release(cc_engine* e, const BatchPass& bp, const TailArgs& ta, const bool batch_assoc, const bool with_publish)
{
    const hipStream_t si = bp.si, sa = bp.sa;
    // (without the host synchronisation behind k_insert_par nobody else reads the counter of k_assocb's stops: four bytes ride along here)
    if (batch_assoc && !bp.gate && !bp.gate2 && e->h_bail_count && !e->capturing)
        CC_HIP_CHECK(e, hipMemcpyAsync(e->h_bail_count, e->d_bail_count, 3 * sizeof(int), hipMemcpyDeviceToHost, sa));
    // Nobody has asked for the id plane (Geometry::publish_ids, cc_engine_output_planes): no pass over the published cells. A pipelined batch
    // then launches nothing here and the events below follow its last association kernel; a captured small call that mirrors its results
    // through k_publish keeps the mirror — one block, whose publish_body returns at once.
    const bool ids = e->g.publish_ids != 0;
    // The ids of the published columns only read what the association of THIS batch left behind (tree root of every cell, cluster id
    // at the root cell; neither is touched again before the ring wraps), so in the pipelined mode they are written on a stream of their
    // own and the next batch's association starts without waiting for them.
    hipStream_t spub = (si != sa && ids) ? e->stream6 : sa;
    if (spub != sa)
    {
        CC_HIP_CHECK(e, hipEventRecord(e->ev_pubrdy[bp.slot], sa));
        CC_HIP_CHECK(e, hipStreamWaitEvent(spub, e->ev_pubrdy[bp.slot], 0));
    }
    if (with_publish && (ids || e->capture_mirror.state))
        hipLaunchKernelGGL(cck::k_publish, ids ? dim3((unsigned) bp.count, cck::PUBLISH_BLOCKS) : dim3(1), dim3(64), 0, spub, e->g, e->P, e->d_states,
                           bp.first_stream, bp.slot, e->capture_mirror);
    CC_MARK(EV_PUBLISH, spub); // ev9: publish
    if (si != sa)
    {
        // the batch descriptor slot is free again after its publish, or — without one — after its last association kernel: nothing behind that reads the descriptor
        CC_HIP_CHECK(e, hipEventRecord(e->ev_assoc[bp.slot], spub));
        e->assoc_pending[bp.slot] = true;
        if (bp.rel_seq)
        {
            // every kernel that reads the call's input buffers is ordered in front of this point (insertion -> segmentation -> association -> publish)
            CC_HIP_CHECK(e, hipEventRecord(e->ev_rel[bp.rel_seq % cc_engine::REL_RING], spub));
            e->rel_recorded[bp.rel_seq % cc_engine::REL_RING] = bp.rel_seq;
        }
    }
    CC_HIP_CHECK(e, hipGetLastError());
    if (e->host_prof && ta.hp_gated)
    {
        e->hp_post += std::chrono::duration<double>(std::chrono::steady_clock::now() - ta.hp_t1).count();
        e->hp_calls++;
    }
    return CC_OK;
}

// ---- small calls: a few firings on ONE stream outside the pipeline (use_small_front) -------------------------------------------------------------
// k_small_front is begin + ego + prep + insertion + segmentation + window scan in one launch; k_small_all is the whole call. Such a call is not
// pipelined, so the pass's five streams are one; the marks of the stages the front kernel absorbed are recorded in a row.
static int launch_small_call(cc_engine* e, const BatchPass& bp, const TailArgs& ta)
{
    const Geometry& g = e->g;
    const hipStream_t s = bp.si;
    int rcp = ensure_prep(e, (size_t) bp.n * g.num_rows);
    if (rcp)
        return rcp;
    const Planes Pf = planes_with_prep(e, bp.prep_buf);
    const bool lean = bp.rpl == 1 && e->assoc_batch && e->assoc_waves >= 2 && e->cfg.cluster_point_trees_every_nth_column == 1 && e->capture_mirror.state != nullptr;
    // the whole call in one launch where the results go to pinned memory (the captured graph of cc_engine_add_firings' small calls): the
    // serial fall-backs, needed once in a long while, are launched by the host when the kernel asks for them (add_firings_small)
    if (e->small_all && lean && e->capture_mirror.tail_req != nullptr)
    {
        hipLaunchKernelGGL(cck::k_small_all, dim3(1), dim3(cck::AB_THREADS), cck::insert2_lds_bytes(g.num_rows), s, g, e->cfg, Pf, e->d_states, bp.first_stream,
                           bp.slot, bp.d_xyz, bp.d_int, bp.d_pose, (long long) bp.n, e->d_remaining, bp.d_ego, e->d_bail_count, e->capture_mirror);
        CC_HIP_CHECK(e, hipGetLastError());
        return CC_OK;
    }
    hipLaunchKernelGGL(cck::k_small_front, dim3(1), dim3(256), cck::insert2_lds_bytes(g.num_rows), s, g, e->cfg, Pf, e->d_states, bp.first_stream, bp.slot, bp.d_xyz,
                       bp.d_int, bp.d_pose, (long long) bp.n, e->d_remaining, bp.d_ego);
    CC_MARK(EV_PREP, s);
    CC_MARK(EV_INSERT, s);
    if (!e->capture_mirror.state) // (a small call's graph gets the counter through k_publish's mirror)
        CC_HIP_CHECK(e, hipMemcpyAsync(e->h_remaining, e->d_remaining, sizeof(int), hipMemcpyDeviceToHost, s));
    CC_MARK(EV_CHAIN2, s);
    CC_MARK(EV_SEGMENT, s);
    const AssocPlan plan = plan_association(e, bp, true);
    CC_MARK(EV_SCAN, s); // (k_small_front has scanned the call's columns)
    // a lean small call (k_small_front in front, results mirrored): k_assocb, then ONE kernel for the serial fall-backs, the ids and the mirror
    const bool small_tail = lean && plan.batch_assoc;
    if (small_tail)
    {
        CC_MARK(EV_CHAIN3, s);
        launch_assocb(e, bp);
        CC_MARK(EV_ASSOC_LDS, s);
        hipLaunchKernelGGL(cck::k_small_tail<1>, dim3(1), dim3(cck::A3_THREADS), 0, s, g, e->cfg, e->P, e->d_states, bp.first_stream, bp.slot, e->capture_mirror);
        CC_MARK(EV_ASSOC_GLOBAL, s);
    }
    else
    {
        Geometry gs = g;
        gs.scan_stores_fin = plan.scan_stores_fin;
        int rca = launch_association(e, bp, plan, gs);
        if (rca)
            return rca;
    }
    return publish_and_release(e, bp, ta, plan.batch_assoc, !small_tail);
}

// ---- the chains behind a batch's insertion: launched at once, by the next call (deferred tail) or once the lazy gate has read the counters -------
static int launch_tail(cc_engine* e, const BatchPass& bp, const TailArgs& ta)
{
    if (bp.first_pass && !bp.prep_done && !bp.par && use_small_front(e, bp.count, bp.n, bp.si != bp.sb))
        return launch_small_call(e, bp, ta);
    int rc = enqueue_insert_serial(e, bp, ta);
    if (rc || (rc = launch_segmentation(e, bp, ta)))
        return rc;
    // (the plan first: it reads the counter of k_assocb's stops as of now, and the scan needs to know whether the serial kernels will associate)
    const AssocPlan plan = plan_association(e, bp, false);
    Geometry gs = e->g;
    gs.scan_stores_fin = plan.scan_stores_fin;
    if ((rc = launch_scan(e, bp, choose_scan(e, bp), gs)) || (rc = launch_association(e, bp, plan, gs)))
        return rc;
    return publish_and_release(e, bp, ta, plan.batch_assoc, true);
}

// The lazy gate's held-back half of a batch: wait for its insertion, read its counters, launch the chains behind it — or, if some stream's batch
// was not taken completely (or is not fused), the other insertion kernels / k_table and k_seg_pre first, then the chains, then — a call of
// limit_columns — the continuation passes, and `redo` (the next batch's insertion, which did nothing) once more.
static int settle_lazy_batch(cc_engine* e, const BatchPass& bp, const std::function<int()>* redo)
{
    CC_HIP_CHECK(e, hipEventSynchronize(e->ev_gate[bp.slot]));
    const bool fb = bp.gate_h_left[0] != 0, seg = bp.gate_h_left[1] != 0;
    if (!fb && !seg)
    {
        e->lazy_miss = 0;
        return launch_tail(e, bp, TailArgs{false, false, true, false, {}});
    }
    if (++e->lazy_miss >= 2)
        e->lazy_ok = false; // (streams that are not in the steady single-column shape: the plain gate from now on)
    int rc = launch_tail(e, bp, TailArgs{fb, seg, false, false, {}});
    if (!rc && hipStreamSynchronize(bp.si) != hipSuccess)
        rc = CC_ERR_HIP;
    if (!rc && *e->h_remaining != 0)
    {
        // the continuation passes go through finish_batch -> launch_batch(e->last_* ...), which fills its pass from the engine: inside the next
        // call's launch_batch those fields are the next batch's already, so this batch's values are put back around it
        const int64_t keep_ntotal = e->cur_ntotal, keep_f0 = e->cur_f0;
        const int keep_buf = e->prep_buf;
        e->cur_ntotal = bp.cur_ntotal, e->cur_f0 = bp.cur_f0, e->prep_buf = bp.prep_buf;
        rc = finish_batch(e);
        e->cur_ntotal = keep_ntotal, e->cur_f0 = keep_f0, e->prep_buf = keep_buf;
    }
    if (!rc && redo)
    {
        e->lazy_redone++;
        rc = (*redo)();
    }
    return rc;
}

// One pass over a batch: insertion on `si`, table + segmentation on `sb`, window scan on `sc`, association + publish on `sa`
// (all equal when not pipelined). What goes onto which stream is in the stages above; this function decides which of them run now,
// which are held back for the next call, and what the host waits for in between.
int launch_batch(cc_engine* e, int first_stream, int count, int64_t n, const float* d_xyz, const uint8_t* d_int,
                 const double* d_pose, bool first_pass, int slot, hipStream_t si, hipStream_t sb, hipStream_t sa,
                 hipStream_t sc = nullptr, hipStream_t sp = nullptr, bool prep_done = false)
{
    e->idle = false;
    int rc = ensure_ego(e, (size_t) count * (size_t) n);
    if (rc)
        return rc;
    const Geometry& g = e->g;
    const auto hp_t0 = std::chrono::steady_clock::now();
    BatchPass bp{};
    bp.si = si, bp.sb = sb, bp.sa = sa;
    bp.sc = sc ? sc : sb; // window scan on the segmentation chain unless the four-stage pipeline gives it its own stream
    bp.slot = slot, bp.first_stream = first_stream, bp.count = count, bp.n = n;
    bp.d_xyz = d_xyz, bp.d_int = d_int, bp.d_pose = d_pose;
    bp.first_pass = first_pass, bp.prep_done = prep_done;
    bp.rpl = (g.num_rows + WAVE - 1) / WAVE;
    bp.cur_ntotal = e->cur_ntotal, bp.cur_f0 = e->cur_f0, bp.prep_buf = e->prep_buf;
    bp.Pt = e->P;
    bp.Pt.tabc += (size_t) slot * (size_t) g.num_streams * (size_t) g.tab_tiles * (size_t) g.num_rows;
    bp.d_ego = e->d_ego[slot];
    bp.gate_left = e->d_par_left + 2 * slot;
    bp.gate_h_left = e->h_par_left + 2 * slot;
    // ---- insertion chain -----------------------------------------------------------------------------------------
    // The head of the batch that has the single-column firing shape is inserted by all wavefronts of a block at once, straight from
    // the caller's buffers; preparation and the serial kernel then only see what is left (StreamState::cursor).
    bp.par = first_pass && !prep_done && e->parallel_insert && n >= 64; // (small calls are latency-bound: one kernel less)
    bp.sp = (bp.par || !sp) ? si : sp; // preparation on the insertion chain unless it runs ahead on its own stream
    // skip_idle_fallbacks: in steady state k_insert_par takes whole batches and the three kernels behind it (k_insert_multi, k_prep, k_insert2)
    // have nothing to do — but their blocks wait for free CUs next to the throughput kernels of the other chains, 0.2 - 0.4 ms of chain time per
    // batch. The host has to wait for the insertion chain before the next batch anyway, so it waits here, for k_insert_par alone, and launches the
    // others only if some stream's batch was not taken completely (the kernel then leaves the batch descriptor to k_insert2 as before).
    // (with the fused segmentation also outside the pipelined mode: the fused path needs the counters the gate reads)
    bp.gate = bp.par && bp.rpl == 1 && (si != sb || e->fuse_front) && e->skip_idle_fallbacks && n <= cck::IP_MAXF && !e->capturing;
    // (above 64 rows k_insert_multi is the first insertion kernel, and the gate is behind it: enqueue_insert_multi)
    bp.gate2 = bp.par && bp.rpl > 1 && e->parallel_insert_multi && si != sb && e->skip_idle_fallbacks;
    // Few streams: a step is as long as its insertion chain PLUS the host's launches of the other chains, because the host waits at the gate
    // before it launches them and the next batch's insertion only starts behind all of that. So the chains behind the gate (launch_tail) of a
    // batch that needs nothing more on the insertion stream are held back and launched by the NEXT call, after that call has enqueued its own
    // insertion and before it waits at its gate: the insertion kernels run back to back and the launches hide behind them. Anything that waits
    // for or reads results launches the held-back chains first (flush_deferred in sync_all).
    // (launches of many streams only defer together with the lazy gate: that pair is what was measured there)
    bp.may_defer = bp.gate && first_pass && si != sb && si != sa && e->defer_tail_max_streams > 0 &&
                   (count <= e->defer_tail_max_streams || (lazy_many_streams(e, count) && lazy_eligible(e, count, n, true, prep_done)));
    bp.lazy = bp.may_defer && lazy_eligible(e, count, n, true, prep_done);
    bp.fuse = bp.gate && e->fuse_front;
    bp.rel_seq = (first_pass && e->in_submit && e->cur_call_last) ? e->call_seq : 0ull;
    bp.mark = e->timing && (e->timing_every <= 1 || e->timing_pass % (uint64_t) e->timing_every == 0);
    if (e->timing)
        e->timing_pass++;
    if (bp.mark && (rc = take_timing_events(e, bp.ev)))
        return rc;
    CC_MARK(EV_START, bp.sp); // ev0
    if (!bp.gate && (rc = flush_deferred(e)))
        return rc;
    TailArgs ta{true, true, false, false, hp_t0};
    if (bp.lazy)
    {
        // this batch's insertion goes out before the previous one's counters have been read
        if ((rc = enqueue_fused_insertion(e, bp, e->lazy_pending ? e->lazy_prev_left : nullptr, true)))
            return rc;
        e->lazy_batches += e->lazy_pending ? 1 : 0;
        CC_MARK(EV_PREP, bp.sp); // ev1
        CC_MARK(EV_INSERT, si);  // ev2
        // now the previous batch: its counters, the chains behind its insertion — or, if it needs the other insertion kernels, those first and
        // then this batch's insertion once more (the one above did nothing)
        const std::function<int()> redo = [e, &bp]() -> int
        {
            hipLaunchKernelGGL(k_begin_batch, dim3((bp.count + 255) / 256), dim3(256), 0, bp.si, e->d_states, bp.first_stream, bp.count, e->d_remaining, 1, bp.slot,
                               (const int*) nullptr, bp.gate_left);
            return enqueue_fused_insertion(e, bp, nullptr, true);
        };
        if ((rc = flush_deferred(e, &redo)))
            return rc;
        e->idle = false; // (the previous batch's closure may have gone through finish_batch / sync_all: this batch's insertion is in flight)
        // whether this batch needs the other insertion kernels, k_table or k_seg_pre, the closure finds out (settle_lazy_batch)
        e->deferred_tail = [e, bp](const std::function<int()>* redo_next) -> int { return settle_lazy_batch(e, bp, redo_next); };
        e->lazy_pending = true;
        e->lazy_prev_left = bp.gate_left;
        return CC_OK;
    }
    if (bp.par && bp.rpl == 1) // (two rows per lane = sensors with per-laser azimuth offsets in practice: straight to k_insert_multi)
    {
        if ((rc = enqueue_fused_insertion(e, bp, nullptr, false)))
            return rc;
        if (bp.gate)
        {
            // (this batch's insertion is enqueued: now the chains of the previous batch that were held back)
            if ((rc = flush_deferred(e)) || (rc = wait_host_gate(e, bp, hp_t0, ta)))
                return rc;
            ta.fallbacks = bp.gate_h_left[0] != 0;
            ta.need_segpre = bp.gate_h_left[1] != 0;
            // an engine that lost the lazy gate (two misses in a row: start-up, sub-rotation batches) gets it back after eight batches in the
            // steady shape; one more miss then switches it off again at once
            if (!e->lazy_ok)
            {
                e->lazy_clean = (ta.fallbacks || ta.need_segpre) ? 0 : e->lazy_clean + 1;
                if (e->lazy_clean >= 8)
                    e->lazy_ok = true, e->lazy_miss = 1, e->lazy_clean = 0;
            }
        }
    }
    if (bp.par && e->parallel_insert_multi && ta.fallbacks && (rc = enqueue_insert_multi(e, bp, hp_t0, ta)))
        return rc;
    if (bp.may_defer && !ta.fallbacks && !ta.need_segpre && !e->capture_mirror.state)
    {
        // what the held-back chains would still put on the insertion stream is put there now (time marks, the early-stop counter, the event the
        // segmentation chain waits for): the held-back part must not touch that stream, the next batch's insertion will be on it by then
        CC_MARK(EV_PREP, bp.sp); // ev1
        CC_MARK(EV_INSERT, si);  // ev2
        CC_HIP_CHECK(e, hipMemcpyAsync(e->h_remaining, e->d_remaining, sizeof(int), hipMemcpyDeviceToHost, si));
        CC_HIP_CHECK(e, hipEventRecord(e->ev_ins[slot], si));
        ta.pre_done = true;
        e->deferred_tail = [e, bp, ta](const std::function<int()>*) -> int { return launch_tail(e, bp, ta); };
        return CC_OK;
    }
    return launch_tail(e, bp, ta);
}
#undef CC_MARK
