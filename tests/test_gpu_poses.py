"""GPU: the pose kernels (include/cc_poses.h) against their host twin, bit for bit, over the track table of
tests/pose_tracks.py; the refusals with a live handle; the device poses chained into an engine against the oracle fed the twin's poses;
replay(poses="device") against replay(poses="twin").

The output arrays of the ABI are dense, [S][n * repeat][12]: between two streams' slices there is no room for a sentinel. The guards sit in
front of the first slice and behind the last; that no stream writes into another's slice shows in every slice being equal to its twin."""
import copy

import numpy as np
import pytest

import cases
import pose_tracks as pt
import util
from continuous_clustering_amd import EngineError, capi, kitti, poses

pytestmark = pytest.mark.gpu

S = 3
GUARD = 24                     # doubles (and stamps) in front of and behind an output array: 192 bytes, keeps the 16-byte alignment
SENTINEL = -7.25e300
STAMP_SENTINEL = 0x5EA5EA5EA5EA5EA5
_shared = {}


def _tracks():
    """Stream 0: one sample; stream 1: two samples about 170 degrees apart; stream 2: the whole table as one track of max_samples samples."""
    if not _shared:
        t = pt.tracks()
        three = [t["single"], (t["near170"][0][:2], t["near170"][1][:2]), pt.combined()]
        _shared.update(tracks=three, queries=[pt.queries(s) for s, _ in three])
    return _shared["tracks"], _shared["queries"]


@pytest.fixture()
def handle():
    tracks, _ = _tracks()
    h = poses.PoseTracks(S, len(tracks[2][0]))
    for s, (st, p) in enumerate(tracks):
        h.set(s, st, p)
    yield h
    h.close()


def _queries_for(n):
    """[S][n] query stamps: the table's queries of each stream's track, all of them when n allows (repeated), evenly picked otherwise."""
    _, queries = _tracks()
    out = np.zeros((S, n), dtype=np.uint64)
    for s, q in enumerate(queries):
        out[s] = np.resize(q, n) if n >= len(q) else q[np.linspace(0, len(q) - 1, n).astype(int)]
    return out


def _guarded(torch, count, dtype, sentinel):
    """A device array of `count` elements between two guards: (whole tensor, pointer of the interior)."""
    whole = torch.full((count + 2 * GUARD,), sentinel, dtype=dtype, device="cuda")
    return whole, whole.data_ptr() + GUARD * whole.element_size()


def _interior(whole, sentinel_bits, kind):
    """The interior as numpy after checking that both guards still hold the sentinel."""
    a = whole.cpu().numpy().view(np.uint64)
    assert (a[:GUARD] == sentinel_bits).all() and (a[-GUARD:] == sentinel_bits).all(), f"{kind}: a guard was overwritten"
    return a[GUARD:-GUARD]


SENTINEL_BITS = np.array([SENTINEL]).view(np.uint64)[0]


@pytest.mark.parametrize("n", [2, 65, 2200])
def test_lookup_equals_the_twin_bit_for_bit(handle, n):
    import torch
    tracks, _ = _tracks()
    q = _queries_for(n)
    want = np.stack([poses.host_lookup(st, p, q[s]) for s, (st, p) in enumerate(tracks)])          # [S][n][12]
    if n == 2200:
        assert len(pt.queries(tracks[2][0])) <= n                                                   # the whole table is in
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    for repeat in (1, 3, 16):
        whole, ptr = _guarded(torch, S * n * repeat * 12, torch.float64, SENTINEL)
        torch.cuda.synchronize()
        handle.lookup(n, d_q, ptr, repeat=repeat)
        handle.sync()
        got = _interior(whole, SENTINEL_BITS, "poses").view(np.float64).reshape(S, n, repeat, 12)
        for r in range(repeat):
            util.assert_float_equal(f"lookup n={n} repeat={repeat} copy {r}", got[:, :, r], want)


@pytest.mark.parametrize("n", [2, 65, 2200])
def test_sweep_equals_the_twin_bit_for_bit_with_and_without_hold(handle, n):
    import torch
    tracks, _ = _tracks()
    start = np.array([max(0, int(st[0]) - 40_000_000) for st, _ in tracks], dtype=np.uint64)   # (stream 1's stamps begin near 0)
    end = np.array([int(st[-1]) + 40_000_000 for st, _ in tracks], dtype=np.uint64)
    twin = [poses.host_sweep(st, p, n, start[s], end[s]) for s, (st, p) in enumerate(tracks)]
    for hold in (None, [-1, 1, -1], [0, -1, 17]):
        want_p = np.stack([tw[1] for tw in twin])
        if hold is not None:
            for s, k in enumerate(hold):
                if k >= 0:
                    want_p[s] = np.tile(tracks[s][1][k], (n, 1))
        for with_stamps in (True, False):
            whole_p, ptr_p = _guarded(torch, S * n * 12, torch.float64, SENTINEL)
            whole_s, ptr_s = _guarded(torch, S * n, torch.int64, STAMP_SENTINEL)
            torch.cuda.synchronize()
            handle.sweep(n, start, end, ptr_p, hold=hold, d_stamps=ptr_s if with_stamps else None)
            handle.sync()
            got_p = _interior(whole_p, SENTINEL_BITS, "poses").view(np.float64).reshape(S, n, 12)
            util.assert_float_equal(f"sweep n={n} hold={hold}", got_p, want_p)
            got_s = _interior(whole_s, np.uint64(STAMP_SENTINEL), "stamps").reshape(S, n)
            if with_stamps:
                assert np.array_equal(got_s, np.stack([tw[0] for tw in twin]))
            else:
                assert (got_s == np.uint64(STAMP_SENTINEL)).all()
    if n == 2200:   # the sweep meets slerp, clamps at both ends and sample stamps
        assert {pt.classify(*tracks[2], int(x)) for x in twin[2][0][::7]} >= {"clamped", "slerp"}


def test_a_second_set_changes_that_stream_only(handle):
    import torch
    tracks, _ = _tracks()
    n = 65
    q = _queries_for(n)
    d_q = torch.from_numpy(q.view(np.int64)).cuda()
    d_before = torch.full((S, n, 12), SENTINEL, dtype=torch.float64, device="cuda")
    d_after = torch.full((S, n, 12), SENTINEL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    handle.lookup(n, d_q, d_before)
    st, p = pt.tracks()["through_pi"]
    st = st - st[0] + tracks[1][0][0]                       # a longer track over the same stamps' neighbourhood
    handle.set(1, st, p)                                    # ordered behind the first lookup on the handle's stream
    handle.lookup(n, d_q, d_after)
    handle.sync()
    before, after = d_before.cpu().numpy(), d_after.cpu().numpy()
    for s in (0, 2):
        util.assert_float_equal(f"stream {s}", after[s], before[s])
    util.assert_float_equal("stream 1 before", before[1], poses.host_lookup(*tracks[1], q[1]))
    util.assert_float_equal("stream 1 after", after[1], poses.host_lookup(st, p, q[1]))
    assert not np.array_equal(before[1], after[1])
    handle.set(1, st[:1], p[:1])                            # a shorter one: the old samples behind it are not met
    handle.lookup(n, d_q, d_after)
    handle.sync()
    util.assert_float_equal("stream 1 shortened", d_after.cpu().numpy()[1], np.tile(p[0], (n, 1)))


def test_refusals_with_a_live_handle_launch_nothing(handle):
    import torch
    tracks, _ = _tracks()
    n = 8
    d_p = torch.full((S, n * 2, 12), SENTINEL, dtype=torch.float64, device="cuda")
    d_s = torch.full((S, n), STAMP_SENTINEL, dtype=torch.int64, device="cuda")
    d_q = torch.from_numpy(_queries_for(n).view(np.int64)).cuda()
    torch.cuda.synchronize()
    start = np.array([int(st[0]) for st, _ in tracks], dtype=np.uint64)
    end = start + np.uint64(1000)
    bad = capi.CC_ERR_INVALID_ARGUMENT
    L = handle.L

    def refused(rc, name):
        assert rc == bad and name.encode() in L.cc_poses_last_error(), (name, rc, L.cc_poses_last_error())

    refused(handle.sweep_raw(1, start, end, d_p), "cc_pose_tracks_sweep")
    refused(handle.sweep_raw(0, start, end, d_p), "cc_pose_tracks_sweep")
    refused(handle.sweep_raw(n, start, end, d_p.data_ptr() + 8), "cc_pose_tracks_sweep")             # misaligned
    refused(handle.sweep_raw(n, start, end, None), "cc_pose_tracks_sweep")
    refused(handle.sweep_raw(n, end, start, d_p), "cc_pose_tracks_sweep")                            # ends before it starts
    refused(handle.sweep_raw(n, start, end, d_p, hold=[-1, 2, -1]), "cc_pose_tracks_sweep")          # stream 1 has samples 0 and 1
    refused(handle.sweep_raw(n, start, end, d_p, hold=[-2, 0, -1]), "cc_pose_tracks_sweep")
    refused(L.cc_pose_tracks_sweep(handle.h, n, None, end.ctypes.data, None, d_p.data_ptr(), None), "cc_pose_tracks_sweep")
    refused(handle.lookup_raw(0, d_q, d_p), "cc_pose_tracks_lookup")
    refused(handle.lookup_raw(n, d_q, d_p, repeat=0), "cc_pose_tracks_lookup")
    refused(handle.lookup_raw(2 ** 30, d_q, d_p, repeat=2), "cc_pose_tracks_lookup")
    refused(handle.lookup_raw(n, d_q, d_p.data_ptr() + 8), "cc_pose_tracks_lookup")                  # misaligned
    refused(handle.lookup_raw(n, None, d_p), "cc_pose_tracks_lookup")
    refused(handle.lookup_raw(n, d_q, None), "cc_pose_tracks_lookup")
    st, p = tracks[2]
    for args in ((3, st, p), (-1, st, p), (0, st[:0], p[:0]), (0, st[::-1], p), (0, np.concatenate([st, st[-1:]]), np.concatenate([p, p[-1:]]))):
        with pytest.raises(EngineError) as e:                # no such stream (twice), no sample, decreasing stamps, more than max_samples
            handle.set(*args)
        assert e.value.code == bad and "cc_pose_tracks_set" in str(e.value)
    refused(L.cc_pose_tracks_set(handle.h, 0, 2, None, p.ctypes.data), "cc_pose_tracks_set")
    handle.sync()
    assert (d_p.cpu().numpy() == SENTINEL).all() and (d_s.cpu().numpy() == STAMP_SENTINEL).all()
    # a stream whose track was never set
    fresh = poses.PoseTracks(2, 4)
    fresh.set(0, st[:3], p[:3])
    refused(fresh.sweep_raw(n, start[:2], end[:2], d_p), "cc_pose_tracks_sweep")
    refused(fresh.lookup_raw(n, d_q, d_p), "cc_pose_tracks_lookup")
    fresh.sync()
    fresh.close()
    assert (d_p.cpu().numpy() == SENTINEL).all()
    # the refusals have not spoilt the handle, and the failed sets have left the tracks alone
    handle.lookup(n, d_q, d_p)
    handle.sync()
    want = np.stack([poses.host_lookup(s_, p_, _queries_for(n)[s]) for s, (s_, p_) in enumerate(tracks)])
    util.assert_float_equal("after the refusals", d_p.cpu().numpy().reshape(-1)[: S * n * 12].reshape(S, n, 12), want)


def _published_in(engine, ev):
    pub = ev[(ev["type"] == capi.EV_PUBLISH_COLUMNS) & (ev["b"] >= ev["a"])]
    if not len(pub):
        return None
    lo, hi = int(pub["a"].min()), int(pub["b"].max())
    return lo, hi, engine.read_columns(lo, hi)


def test_device_sweep_chained_into_an_engine_equals_the_oracle_fed_the_twins_poses(oracle_lib):
    """A synthetic stream of tests/cases.py whose poses are a sweep over a track: xyz and intensity uploaded, d_poses written by `sweep` on
    the engine's HIP stream, fed 64 firings per call; events, published columns and state against the oracle fed the twin's poses."""
    import torch
    from continuous_clustering_amd import Engine, IDENTITY_TF
    stream, cfg, tf = cases.build_case("g_s64_translate")
    tf = IDENTITY_TF if tf is None else tf
    n = stream.n_firings
    # the track: the stream's own motion sampled every 100 firings (100 ms apart), with a yaw that grows by 0.01 rad per sample on top
    at = list(range(0, n, 100)) + [n - 1]
    t_stamps = np.array([pt.EPOCH + 1_000_000 * k for k in at], dtype=np.uint64)
    t_poses = np.stack([pt.pose(pt.rot(2, 0.01 * i) @ stream.poses[k].reshape(3, 4)[:, :3], stream.poses[k].reshape(3, 4)[:, 3]) for i, k in enumerate(at)])
    start, end = int(t_stamps[0]) - 20_000_000, int(t_stamps[-1]) + 20_000_000    # the sweep begins before the first sample and ends behind the last
    _, twin = poses.host_sweep(t_stamps, t_poses, n, start, end)
    assert "slerp" in {pt.classify(t_stamps, t_poses, int(t_stamps[1]) + 5), pt.classify(t_stamps, t_poses, int(t_stamps[3]) + 5)}
    fed = copy.copy(stream)
    fed.poses = twin
    oracle, rc = util.run_oracle(fed, cfg, tf)
    assert rc == 0
    evo = oracle.drain_events()
    lo, hi = oracle.published_range()
    assert (evo["type"] == capi.EV_CLUSTER).sum() > 5 and hi - lo > 100

    e = Engine(cfg, 64, 1, 0, tf)
    e.record_events(True)
    e.set_option("input_on_engine_stream", 1)
    tracks = poses.PoseTracks(1, len(t_stamps), hip_stream=e.hip_stream())
    tracks.set(0, t_stamps, t_poses)
    d_xyz = torch.from_numpy(stream.xyz).cuda()
    d_int = torch.from_numpy(stream.intensity).cuda()
    d_pose = torch.full((1, n, 12), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    tracks.sweep(n, [start], [end], d_pose)                                       # not waited for: the engine's calls are behind it on the stream
    events, pieces = [], []
    for f0 in range(0, n, 64):
        m = min(64, n - f0)
        e.add_firings_device(m, d_xyz[f0:f0 + m], d_int[f0:f0 + m], d_pose[0, f0:f0 + m])
        assert e.sync() == 0, e.last_error()
        events.append(e.drain_events())
        pieces.append(_published_in(e, events[-1]))
    util.assert_float_equal("device poses", d_pose.cpu().numpy()[0], twin)
    ev = np.concatenate(events)
    assert len(ev) == len(evo)
    for fld in ("type", "a", "b", "c", "d", "column"):
        assert np.array_equal(ev[fld], evo[fld]), fld
    pieces = [p for p in pieces if p is not None]
    assert pieces[0][0] == lo and pieces[-1][1] == hi and all(a[1] + 1 == b[0] for a, b in zip(pieces, pieces[1:]))
    util.compare_columns(oracle.read_published(lo, hi), {k: np.concatenate([p[2][k] for p in pieces]) for k in pieces[0][2]}, lo)
    so, se = oracle.state(), e.state()
    for k in util.STATE_FIELDS:
        assert so[k] == se[k], k
    tracks.close()                                                                # before the engine whose HIP stream it uses
    e.close()


def test_replay_with_device_poses_equals_replay_with_the_twin(tmp_path):
    """Three sequences of different lengths (the shorter ones end early and are held at their last pose): poses="device" gives exactly the
    records and totals of poses="twin". Equality with poses="host" is printed, not asserted: the two differ by the libm."""
    from continuous_clustering_amd import replay
    from continuous_clustering_amd.evaluation import gather_records
    lengths = {2: 3, 4: 2, 7: 4}
    for k, (seq, nf) in enumerate(lengths.items()):
        kitti.write_synthetic_sequence(str(tmp_path), seq, nf, seed=100 + 10 * k, motion=(6.0 + k, 0.1 * k, 0.0, 0.1 * (k + 1)))
    got = {}
    for mode in ("twin", "device", "host"):
        records, totals = replay.replay(str(tmp_path), list(lengths), poses=mode)
        got[mode] = (gather_records(records), totals)
    rec_t, tot_t = got["twin"]
    rec_d, tot_d = got["device"]
    assert tot_t["streams"] == 3 and tot_t["frames"] == sum(lengths.values()) and len(rec_t) == sum(lengths.values())
    assert tot_d == tot_t
    assert rec_d.shape == rec_t.shape and np.array_equal(rec_d.view(np.uint64), rec_t.view(np.uint64))
    rec_h, tot_h = got["host"]
    same = rec_h.shape == rec_d.shape and np.array_equal(rec_h.view(np.uint64), rec_d.view(np.uint64))
    print(f"poses='host' against poses='device': records {'equal' if same else 'differ'}, totals {'equal' if tot_h == tot_d else 'differ'}")
