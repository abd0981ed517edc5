"""The firing-stamp log (include/cc_stamps.h) in plain Python / numpy, written from the reference's lines and not from the
library's text, and the synthetic record arrays both stamp test files run through the host twins and the kernels.

* resolution: a model that REMEMBERS every pushed firing under its full 64-bit index and looks a 32-bit key up among the firings the log
  still holds (the newest `capacity`, none from before a seek) - no ring, no modular trick;
* cluster stamp: cc.cpp:1007-1010 (min / max over all members, zeros included) and 1025-1028 (max, or min + (max - min) / 2);
* column / message stamp: ros_utils.cpp:51-71 (minimum non-zero stamp; 0 where there is none);
* time_sec / time_nsec: ros::Time::fromNSec (ros_utils.cpp:251-266).
"""
import numpy as np

from continuous_clustering_amd import take
from continuous_clustering_amd.stamps import CLUSTER_STAMP_DTYPE

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
BASE = 1_700_000_000_000_000_000
EARLIEST = BASE - 300_000   # what jittered() can fall to


class ModelLog:
    def __init__(self, num_streams, capacity):
        self.S, self.capacity = num_streams, capacity
        self.held = [dict() for _ in range(num_streams)]   # full firing index -> stamp, everything since the last seek / reset
        self.heads = [0] * num_streams
        self.missing = [0] * num_streams

    def push_host(self, stream, stamps):
        for v in np.asarray(stamps, dtype=np.uint64).reshape(-1):
            self.held[stream][self.heads[stream]] = int(v)
            self.heads[stream] += 1

    def push(self, stamps, repeat=1):
        stamps = np.asarray(stamps, dtype=np.uint64).reshape(self.S, -1)
        for s in range(self.S):
            self.push_host(s, np.repeat(stamps[s], repeat))

    def seek(self, stream, next_firing):
        self.held[stream], self.heads[stream] = {}, int(next_firing)

    def reset_streams(self, streams):
        for s in ([streams] if isinstance(streams, int) else streams):
            self.held[s], self.heads[s], self.missing[s] = {}, 0, 0

    def counters(self, stream=0):
        return self.heads[stream], self.missing[stream]

    def resolve(self, stream, f):
        """(stamp, missing) of the newest firing the log still holds whose index has the low 32 bits f"""
        head, f = self.heads[stream], int(f)
        if head == 0:
            return 0, True
        idx = ((head - 1) >> 32 << 32) | f
        if idx > head - 1:
            idx -= 1 << 32
        if idx < 0 or idx < head - self.capacity or idx not in self.held[stream]:
            return 0, True
        return self.held[stream][idx], False


def sec_nsec(stamp):
    return (int(stamp) // 10 ** 9) & M32, int(stamp) % 10 ** 9


def model_of_points(log, rec, table):
    stamps = np.zeros(len(rec), dtype=np.uint64)
    for s in range(log.S):
        a, n = int(table[s]["first_record"]), int(table[s]["n_records"])
        for i in range(a, a + n):
            v, miss = log.resolve(s, rec["source_firing"][i])
            stamps[i] = v
            log.missing[s] += miss
    sn = np.array([sec_nsec(v) for v in stamps], dtype=np.uint32).reshape(-1, 2)
    return stamps, sn


def nonzero_min(values):
    values = [int(v) for v in values if int(v) != 0]
    return min(values) if values else 0


def model_of_columns(log, rec, table):
    """column stamps ordered by stream then column, stream stamps; counts missing like model_of_points"""
    stamps, _ = model_of_points(log, rec, table)
    cols, streams = [], []
    for s in range(log.S):
        a, n = int(table[s]["first_record"]), int(table[s]["n_records"])
        mine, col = stamps[a:a + n], rec["column"][a:a + n]
        for c in range(max(int(table[s]["col_to"] - table[s]["col_from"]), 0)):
            cols.append(nonzero_min(mine[col == c]))
        streams.append(nonzero_min(mine))
    return np.array(cols, dtype=np.uint64), np.array(streams, dtype=np.uint64)


def model_of_clusters(log, cl, rec, use_last_point):
    out = np.zeros(len(cl), dtype=CLUSTER_STAMP_DTYPE)
    points = np.zeros(len(rec), dtype=np.uint64)
    for k in range(len(cl)):
        s, a, n = int(cl[k]["stream"]), int(cl[k]["first_record"]), int(cl[k]["n_points"])
        lo, hi, lost = M64, 0, 0                                   # cc.cpp:991-992
        for i in range(a, a + n):
            v, miss = log.resolve(s, rec["source_firing"][i])
            points[i] = v
            lost += miss
            lo, hi = min(lo, v), max(hi, v)                        # cc.cpp:1007-1010: zeros are not skipped
        if n:
            log.missing[s] += lost
            out[k] = (hi if use_last_point else lo + (hi - lo) // 2, lo, hi, lost, 0)   # cc.cpp:1025-1028
    return out, points


# ---- the synthetic case ---------------------------------------------------------------------------------------------------------------------
CAPACITY, S = 1024, 5
WRAP_KEYS = (1975, 1976, 2999, 3000)     # of stream 0 after 3000 pushes into 1024 slots: missing, oldest held, newest, not pushed yet
SEEK_AT = (1 << 32) - 500                # stream 2: seek here, push 1000: held indices straddle 2^32
SPECIAL = [0, (1 << 63) + 10, (1 << 63) + 13, (5 << 32) | 7, (9 << 32) | 7, (5 << 32) | 1000, 1, M64]   # stream 4, firings 8 .. 15
CLUSTER_SIZES = (1, 63, 64, 70001, 65, 4097)


def jittered(rng, n):
    """stamps around 1.7e18 ns, 100 us apart with +-300 us of jitter: not monotonic in the firing index"""
    return (BASE + np.arange(n, dtype=np.int64) * 100_000 + rng.integers(-300_000, 300_000, n)).astype(np.uint64)


def fill_log(log, seed=11):
    """stream 0: 3000 firings through 1024 slots; 1: nothing, head 0; 2: across 2^32; 3: 77 firings; 4: 8 ordinary firings and SPECIAL"""
    rng = np.random.default_rng(seed)
    for part in np.split(jittered(rng, 3000), [1000, 2000]):
        log.push_host(0, part)
    log.seek(2, SEEK_AT)
    log.push_host(2, jittered(rng, 1000))
    log.push_host(3, jittered(rng, 77))
    log.push_host(4, np.concatenate([jittered(rng, 8), np.array(SPECIAL, dtype=np.uint64)]))
    return log


def _keys(rng, stream, n):
    if stream == 0:   # from before the oldest held firing to beyond the head
        k = rng.integers(1900, 3010, n)
        k[:len(WRAP_KEYS)] = WRAP_KEYS[:n]
        return k.astype(np.uint32)
    if stream == 2:   # low 32 bits from both sides of 2^32, a few from before the seek and beyond the head
        return ((SEEK_AT + rng.integers(-40, 1020, n)) & M32).astype(np.uint32)
    return rng.integers(0, 8, n).astype(np.uint32)


def point_case(seed=12):
    """(records, table): 5 streams; 1 and 3 have empty slices (3 has columns all the same); stream 4's columns: stamps, only zeros, zeros mixed
    with stamps, none, SPECIAL"""
    rng = np.random.default_rng(seed)
    counts, widths, col_from = [300, 0, 200, 0, 40], [10, 0, 7, 4, 5], [100, 50, 7, 0, 1 << 40]
    table = np.zeros(S, dtype=take.TAKE_STREAM_DTYPE)
    rec = np.zeros(sum(counts), dtype=take.TAKE_POINT_DTYPE)
    pos = 0
    for s in range(S):
        n = counts[s]
        table[s] = (col_from[s], col_from[s] + widths[s], 0, pos, n, 0, 0)
        if n:
            r = rec[pos:pos + n]
            r["source_firing"] = _keys(rng, s, n)
            if s == 4:
                r["column"] = np.repeat([0, 1, 2, 4], 10)
                r["source_firing"][10:20] = 8                        # column 1: only the firing stamped 0
                r["source_firing"][20:30] = [8, 3, 8, 5, 8, 8, 1, 8, 8, 8]   # column 2: zeros mixed with stamps; column 3: no record
                r["source_firing"][30:40] = [9, 10, 11, 12, 13, 14, 15, 15, 14, 9]
            else:
                cols = np.sort(rng.integers(0, widths[s], n))
                r["column"] = np.where(cols == 3, 4, cols)           # column 3 stays without a record
            r["row"] = rng.integers(0, 64, n)
        pos += n
    return rec, table


def cluster_case(seed=13):
    """(descriptors, records): sizes 1, 63, 64 on stream 0, 70 001 and 65 on stream 2, 4097 and the SPECIAL pairs on stream 4"""
    rng = np.random.default_rng(seed)
    special = [[9, 10, 9], [11, 12], [11, 13], [14, 15, 14], [8, 3, 5], [15]]   # > 2^63 and odd; high words; low words; 1 and 2^64-1; a zero
    layout = [(0, 1), (0, 63), (0, 64), (2, 70001), (2, 65), (4, 4097)] + [(4, len(k)) for k in special]
    cl = np.zeros(len(layout), dtype=take.TAKE_CLUSTER_DTYPE)
    rec = np.zeros(sum(n for _, n in layout), dtype=take.TAKE_POINT_DTYPE)
    pos = 0
    for i, (s, n) in enumerate(layout):
        cl[i]["stream"], cl[i]["id"], cl[i]["first_record"], cl[i]["n_points"], cl[i]["n_columns"] = s, i + 1, pos, n, 1
        rec["source_firing"][pos:pos + n] = _keys(rng, s, n) if i < len(CLUSTER_SIZES) else special[i - len(CLUSTER_SIZES)]
        rec["id"][pos:pos + n] = i + 1
        pos += n
    rec["source_firing"][0] = 2999   # the one-point cluster is held
    return cl, rec


def same(a, b):
    """bit for bit"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes()
