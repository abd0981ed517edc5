// cc_stamps.hip — the firing-stamp log and its three resolve calls on gfx950 (include/cc_stamps.h).
//
// State in device memory: rings [S][capacity] uint64, missing [S], and the streams' {head, floor} TWICE, logs[2][S]. Every call that changes a
// head is one kernel that reads logs[gen & 1] and writes all of logs[(gen + 1) & 1]; the host counts gen. So a push needs no second launch
// to advance the heads and no block reads a head another block of the same launch is writing.
// Resolve kernels: one lane per record everywhere. A record's second half is read as one 16-byte load (id, source_firing, row.., column).
// The record -> stream search (points, columns) is a binary search over the slices' first records, staged in LDS up to LDS_STREAMS streams.
// Columns and clusters reduce inside the wavefront first (a segmented min / max over lanes that share a destination, by shuffles) and then
// issue one 64-bit atomicMin / atomicMax per destination and wavefront into outputs initialised with the identity; a small kernel finishes
// (key + 1 for the non-zero minimum, the midpoint for clusters). Min and max do not depend on the order, so the atomics cost no
// reproducibility. Clusters: a block of 256 consecutive records finds the descriptor of its first record by a 256-ary search over the
// descriptors' first_record, stages the next 257 descriptors in LDS (256 records touch at most 256 non-empty clusters) and every lane
// searches there; a 70 001-point cluster is thus spread over 274 blocks, a 6-point one shares a wavefront with its neighbours.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cc_stamps.h"
#include "cc_stamp_math.h"

namespace
{

thread_local std::string g_stamps_error;

int fail(int code, const std::string& what)
{
    g_stamps_error = what;
    return code;
}

#define STAMPS_HIP_CHECK(expr)                                                                         \
    do                                                                                                 \
    {                                                                                                  \
        hipError_t err__ = (expr);                                                                     \
        if (err__ != hipSuccess)                                                                       \
            return fail(CC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(err__));             \
    } while (0)

typedef unsigned long long ull;
static_assert(sizeof(ull) == sizeof(uint64_t), "64-bit atomics are used on uint64_t");
static_assert(sizeof(cc_take_point) == 32 && sizeof(cc_take_stream) == 48 && sizeof(cc_take_cluster) == 64 && sizeof(cc_cluster_stamp) == 32,
              "record layouts");

constexpr int BLOCK = 256;          // four wavefronts
constexpr int LDS_STREAMS = 1024;   // tables up to this many streams are staged in LDS (8 KiB, 16 with the column offsets)
constexpr uint64_t MAX_CAPACITY = 1ull << 31;
constexpr uint64_t NO_STAMP = ~0ull;

__host__ __device__ inline int64_t columns_of(const cc_take_stream& t)
{
    return t.col_to > t.col_from ? t.col_to - t.col_from : 0;
}

// id, source_firing, row / label / intensity, column of a record
__device__ __forceinline__ uint4 second_half(const cc_take_point* records, int64_t i)
{
    return *(const uint4*) ((const char*) (records + i) + 16);
}

// ---- the log ------------------------------------------------------------------------------------------------------------------------------------

// grid (ceil(n * repeat / BLOCK), S). only < 0: src is [S][n] and every stream pushes; else src is [n] and only that stream does.
__global__ __launch_bounds__(BLOCK) void k_push(const ccs::Log* cur, ccs::Log* next, uint64_t* rings, uint64_t capacity, const uint64_t* src,
                                                 int64_t n, int repeat, int only)
{
    const int s = blockIdx.y;
    const ccs::Log log = cur[s];
    const int64_t total = (only < 0 || s == only) ? n * repeat : 0;
    const int64_t t = (int64_t) blockIdx.x * BLOCK + threadIdx.x;
    if (t < total) // total <= capacity: no two threads meet in a slot
        rings[(size_t) s * capacity + ((log.head + (uint64_t) t) & (capacity - 1))] = src[(only < 0 ? (size_t) s * n : 0) + (size_t) (t / repeat)];
    if (t == 0)
        next[s] = ccs::Log{log.head + (uint64_t) total, log.floor};
}

__global__ __launch_bounds__(BLOCK) void k_seek(const ccs::Log* cur, ccs::Log* next, int S, int stream, uint64_t next_firing)
{
    const int s = blockIdx.x * BLOCK + threadIdx.x;
    if (s < S)
        next[s] = s == stream ? ccs::Log{next_firing, next_firing} : cur[s];
}

__global__ __launch_bounds__(BLOCK) void k_reset(const ccs::Log* cur, ccs::Log* next, ull* missing, int S, const uint8_t* flags)
{
    const int s = blockIdx.x * BLOCK + threadIdx.x;
    if (s >= S)
        return;
    if (flags[s])
        missing[s] = 0;
    next[s] = flags[s] ? ccs::Log{0, 0} : cur[s];
}

// ---- wave-level segmented reductions: lanes that share `seg` and are neighbours reduce into the first of them ----------------------------------
// After the step with distance d a lane holds the reduction over itself and the next 2d - 1 lanes as far as they share its seg. All 64 lanes
// must be active.

__device__ __forceinline__ bool seg_head(int64_t seg, int lane)
{
    const int64_t before = __shfl_up((long long) seg, 1);
    return lane == 0 || before != seg;
}

template <bool MAX>
__device__ __forceinline__ uint64_t seg_minmax(uint64_t v, int64_t seg, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const uint64_t ov = __shfl_down((ull) v, d);
        const int64_t os = __shfl_down((long long) seg, d);
        if (lane + d < 64 && os == seg)
            v = MAX ? (ov > v ? ov : v) : (ov < v ? ov : v);
    }
    return v;
}

__device__ __forceinline__ uint32_t seg_sum(uint32_t v, int64_t seg, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1)
    {
        const uint32_t ov = __shfl_down(v, d);
        const int64_t os = __shfl_down((long long) seg, d);
        if (lane + d < 64 && os == seg)
            v += ov;
    }
    return v;
}

// ---- points -------------------------------------------------------------------------------------------------------------------------------------

template <bool STAGED>
__device__ __forceinline__ int stream_of_record(const int64_t* lds_first, const cc_take_stream* table, int S, int64_t i)
{
    if (STAGED)
        return ccs::slice_of(S, i, [&](int k) { return lds_first[k]; });
    return ccs::slice_of(S, i, [&](int k) { return table[k].first_record; });
}

template <bool STAGED>
__global__ __launch_bounds__(BLOCK) void k_of_points(const ccs::Log* logs, const uint64_t* rings, uint64_t capacity, ull* missing, int S,
                                                      int64_t n, const cc_take_point* records, const cc_take_stream* table, uint64_t* stamps,
                                                      uint2* sec_nsec)
{
    __shared__ int64_t lds_first[STAGED ? LDS_STREAMS : 1];
    if (STAGED)
    {
        for (int s = threadIdx.x; s < S; s += BLOCK)
            lds_first[s] = table[s].first_record;
        __syncthreads();
    }
    const int64_t i = (int64_t) blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n)
        return;
    const uint4 half = second_half(records, i);
    const int s = stream_of_record<STAGED>(lds_first, table, S, i);
    uint64_t stamp = 0;
    if (s >= 0)
    {
        bool miss;
        stamp = ccs::resolve(rings + (size_t) s * capacity, capacity, logs[s], half.y, &miss);
        if (miss)
            atomicAdd(&missing[s], 1ull);
    }
    stamps[i] = stamp;
    if (sec_nsec)
    {
        uint2 t;
        ccs::sec_nsec(stamp, &t.x, &t.y);
        sec_nsec[i] = t;
    }
}

// ---- columns ------------------------------------------------------------------------------------------------------------------------------------

// one block: offsets[s] = sum over t < s of the columns of stream t, offsets[S] = all
__global__ __launch_bounds__(BLOCK) void k_column_offsets(const cc_take_stream* table, int S, int64_t* offsets)
{
    __shared__ int64_t scan[BLOCK];
    __shared__ int64_t carry;
    if (threadIdx.x == 0)
        carry = 0;
    __syncthreads();
    for (int base = 0; base < S; base += BLOCK)
    {
        const int s = base + threadIdx.x;
        const int64_t mine = s < S ? columns_of(table[s]) : 0;
        scan[threadIdx.x] = mine;
        __syncthreads();
        for (int d = 1; d < BLOCK; d <<= 1)
        {
            const int64_t add = threadIdx.x >= d ? scan[threadIdx.x - d] : 0;
            __syncthreads();
            scan[threadIdx.x] += add;
            __syncthreads();
        }
        if (s < S)
            offsets[s] = carry + scan[threadIdx.x] - mine;
        __syncthreads();
        if (threadIdx.x == 0)
            carry += scan[BLOCK - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        offsets[S] = carry;
}

// column_keys [n_columns] and stream_keys [S] hold nonzero_min_key values, initialised to 2^64 - 1; either may be NULL
template <bool STAGED>
__global__ __launch_bounds__(BLOCK) void k_of_columns(const ccs::Log* logs, const uint64_t* rings, uint64_t capacity, ull* missing, int S,
                                                       int64_t n, const cc_take_point* records, const cc_take_stream* table,
                                                       const int64_t* offsets, int64_t n_columns, ull* column_keys, ull* stream_keys)
{
    __shared__ int64_t lds_first[STAGED ? LDS_STREAMS : 1];
    __shared__ int64_t lds_offsets[STAGED ? LDS_STREAMS + 1 : 1];
    if (STAGED)
    {
        for (int s = threadIdx.x; s < S; s += BLOCK)
            lds_first[s] = table[s].first_record;
        for (int s = threadIdx.x; s <= S; s += BLOCK)
            lds_offsets[s] = offsets[s];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t) blockIdx.x * BLOCK + threadIdx.x;
    int64_t stream_seg = -1, column_seg = -1;
    uint64_t key = NO_STAMP;
    if (i < n)
    {
        const uint4 half = second_half(records, i);
        const int s = stream_of_record<STAGED>(lds_first, table, S, i);
        if (s >= 0)
        {
            bool miss;
            key = ccs::nonzero_min_key(ccs::resolve(rings + (size_t) s * capacity, capacity, logs[s], half.y, &miss));
            if (miss)
                atomicAdd(&missing[s], 1ull);
            stream_seg = s;
            const int64_t from = STAGED ? lds_offsets[s] : offsets[s], to = STAGED ? lds_offsets[s + 1] : offsets[s + 1];
            const int64_t at = from + (int64_t) half.w;
            if (at < to && at < n_columns) // (a column outside its stream's range is not a column of this take)
                column_seg = at;
        }
    }
    const uint64_t column_min = seg_minmax<false>(key, column_seg, lane);
    const uint64_t stream_min = seg_minmax<false>(key, stream_seg, lane);
    if (column_keys && column_seg >= 0 && seg_head(column_seg, lane) && column_min != NO_STAMP)
        atomicMin(&column_keys[column_seg], (ull) column_min);
    if (stream_keys && stream_seg >= 0 && seg_head(stream_seg, lane) && stream_min != NO_STAMP)
        atomicMin(&stream_keys[stream_seg], (ull) stream_min);
}

__global__ __launch_bounds__(BLOCK) void k_keys_to_stamps(uint64_t* keys, int64_t n)
{
    const int64_t i = (int64_t) blockIdx.x * BLOCK + threadIdx.x;
    if (i < n)
        keys[i] = ccs::nonzero_min_from_key(keys[i]);
}

// ---- clusters -----------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(BLOCK) void k_clusters_init(cc_cluster_stamp* out, int64_t n)
{
    const int64_t c = (int64_t) blockIdx.x * BLOCK + threadIdx.x;
    if (c < n)
        out[c] = cc_cluster_stamp{0, NO_STAMP, 0, 0, 0};
}

// The cluster that holds record i: the last descriptor with first_record <= i (descriptors abut in order), provided i lies inside it.
__global__ __launch_bounds__(BLOCK) void k_of_clusters(const ccs::Log* logs, const uint64_t* rings, uint64_t capacity, ull* missing, int S,
                                                        int64_t n_clusters, const cc_take_cluster* clusters, int64_t n,
                                                        const cc_take_point* records, cc_cluster_stamp* out, uint64_t* point_stamps)
{
    constexpr int STAGE = BLOCK + 1;
    __shared__ int64_t c_first[STAGE];
    __shared__ uint32_t c_points[STAGE];
    __shared__ int32_t c_stream[STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t block_first = (int64_t) blockIdx.x * BLOCK;

    // 256-ary search for the number of descriptors with first_record <= block_first: all below lo have it, none from hi on
    int64_t lo = 0, hi = n_clusters;
    while (hi - lo > BLOCK)
    {
        const int64_t step = (hi - lo + BLOCK - 1) / BLOCK;
        const int64_t chunk_last = lo + (int64_t) (tid + 1) * step - 1; // the last descriptor of this thread's chunk
        const int whole = __syncthreads_count(chunk_last < hi && clusters[chunk_last].first_record <= block_first);
        const int64_t new_lo = lo + (int64_t) whole * step;
        hi = new_lo + step < hi ? new_lo + step : hi;
        lo = new_lo < hi ? new_lo : hi;
    }
    lo += __syncthreads_count(lo + tid < hi && clusters[lo + tid].first_record <= block_first);
    const int64_t base = lo > 0 ? lo - 1 : 0; // the descriptor of the block's first record, or descriptor 0
    const int staged = (int) (n_clusters - base < STAGE ? n_clusters - base : STAGE);
    for (int k = tid; k < staged; k += BLOCK)
    {
        const cc_take_cluster d = clusters[base + k];
        c_first[k] = d.first_record;
        c_points[k] = d.n_points;
        c_stream[k] = d.stream;
    }
    __syncthreads();

    const int64_t i = block_first + tid;
    int64_t seg = -1;
    uint64_t stamp = 0;
    uint32_t miss_count = 0;
    int stream = -1;
    if (i < n)
    {
        const uint4 half = second_half(records, i);
        int k = ccs::slice_of(staged, i, [&](int j) { return c_first[j]; });
        int64_t first = 0;
        uint32_t points = 0;
        if (k >= 0)
        {
            first = c_first[k];
            points = c_points[k];
            stream = c_stream[k];
            seg = base + k;
        }
        if (k == staged - 1 && base + staged < n_clusters && i >= first + (int64_t) points)
        {   // descriptors without members used up the staged window: search all of them
            seg = ccs::slice_of((int) (n_clusters < INT32_MAX ? n_clusters : INT32_MAX), i, [&](int j) { return clusters[j].first_record; });
            if (seg >= 0)
            {
                first = clusters[seg].first_record;
                points = clusters[seg].n_points;
                stream = clusters[seg].stream;
            }
        }
        if (seg >= 0 && i >= first + (int64_t) points)
            seg = -1; // a record between two clusters
        if (seg >= 0)
        {
            bool miss = true;
            if (stream >= 0 && stream < S)
                stamp = ccs::resolve(rings + (size_t) stream * capacity, capacity, logs[stream], half.y, &miss);
            else
                stream = -1;
            miss_count = miss ? 1 : 0;
            if (point_stamps)
                point_stamps[i] = stamp;
        }
    }
    const uint64_t lowest = seg_minmax<false>(stamp, seg, lane);
    const uint64_t highest = seg_minmax<true>(stamp, seg, lane);
    const uint32_t lost = seg_sum(miss_count, seg, lane);
    if (seg >= 0 && seg_head(seg, lane))
    {
        atomicMin((ull*) &out[seg].min_stamp, (ull) lowest);
        atomicMax((ull*) &out[seg].max_stamp, (ull) highest);
        if (lost)
        {
            atomicAdd(&out[seg].n_missing, lost);
            if (stream >= 0)
                atomicAdd(&missing[stream], (ull) lost);
        }
    }
}

__global__ __launch_bounds__(BLOCK) void k_clusters_finish(cc_cluster_stamp* out, int64_t n, int use_last_point)
{
    const int64_t c = (int64_t) blockIdx.x * BLOCK + threadIdx.x;
    if (c >= n)
        return;
    cc_cluster_stamp r = out[c];
    if (r.min_stamp > r.max_stamp) // untouched: no member
        r = cc_cluster_stamp{0, 0, 0, 0, 0};
    else
        r.stamp = ccs::cluster_stamp(r.min_stamp, r.max_stamp, use_last_point != 0);
    out[c] = r;
}

unsigned blocks_for(int64_t n)
{
    return (unsigned) ((n + BLOCK - 1) / BLOCK);
}

// ---- host twins' helpers --------------------------------------------------------------------------------------------------------------------------

const char* bad_host_log(const cc_stamps_host_log* log)
{
    if (!log || log->num_streams <= 0 || !log->rings || !log->heads || !log->floors || !log->missing)
        return "a log with its four arrays is required";
    if (log->capacity < 1 || (log->capacity & (log->capacity - 1)) != 0)
        return "the log's capacity must be a power of two";
    return nullptr;
}

uint64_t host_resolve(const cc_stamps_host_log* log, int s, uint32_t f, bool* miss)
{
    return ccs::resolve(log->rings + (size_t) s * (size_t) log->capacity, (uint64_t) log->capacity, ccs::Log{log->heads[s], log->floors[s]}, f,
                        miss);
}

} // namespace

struct cc_firing_stamps
{
    int device = 0;
    int num_streams = 0;
    uint64_t capacity = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint64_t* d_rings = nullptr;      // [S][capacity]
    ccs::Log* d_logs = nullptr;       // [2][S]; [gen & 1] is current
    unsigned gen = 0;
    ull* d_missing = nullptr;         // [S]
    int64_t* d_offsets = nullptr;     // [S + 1], scratch of cc_firing_stamps_of_columns
    unsigned char* h_stage = nullptr; // pinned: the stamps of a push_host, or the flags of a reset
    unsigned char* d_stage = nullptr;
    size_t stage_bytes = 0;
    hipEvent_t stage_done = nullptr;  // the upload out of h_stage has run
    bool stage_pending = false;
    std::vector<cc_take_stream> table; // of_columns without h_table

    const ccs::Log* cur() const { return d_logs + (size_t) (gen & 1) * num_streams; }
    ccs::Log* next() const { return d_logs + (size_t) ((gen + 1) & 1) * num_streams; }
};

namespace
{

void release(cc_firing_stamps* h)
{
    (void) hipSetDevice(h->device);
    if (h->stream)
        (void) hipStreamSynchronize(h->stream);
    for (void* p : {(void*) h->d_rings, (void*) h->d_logs, (void*) h->d_missing, (void*) h->d_offsets, (void*) h->d_stage})
        if (p)
            (void) hipFree(p);
    if (h->h_stage)
        (void) hipHostFree(h->h_stage);
    if (h->stage_done)
        (void) hipEventDestroy(h->stage_done);
    if (h->own_stream && h->stream)
        (void) hipStreamDestroy(h->stream);
    delete h;
}

int create(cc_firing_stamps* h, void* hip_stream)
{
    STAMPS_HIP_CHECK(hipSetDevice(h->device));
    if (hip_stream)
        h->stream = (hipStream_t) hip_stream;
    else
    {
        STAMPS_HIP_CHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
        h->own_stream = true;
    }
    const size_t S = (size_t) h->num_streams;
    h->stage_bytes = h->capacity * sizeof(uint64_t) > S ? h->capacity * sizeof(uint64_t) : S;
    STAMPS_HIP_CHECK(hipMalloc(&h->d_rings, S * h->capacity * sizeof(uint64_t)));
    STAMPS_HIP_CHECK(hipMalloc(&h->d_logs, 2 * S * sizeof(ccs::Log)));
    STAMPS_HIP_CHECK(hipMalloc(&h->d_missing, S * sizeof(ull)));
    STAMPS_HIP_CHECK(hipMalloc(&h->d_offsets, (S + 1) * sizeof(int64_t)));
    STAMPS_HIP_CHECK(hipMalloc(&h->d_stage, h->stage_bytes));
    STAMPS_HIP_CHECK(hipHostMalloc(&h->h_stage, h->stage_bytes, hipHostMallocDefault));
    STAMPS_HIP_CHECK(hipEventCreateWithFlags(&h->stage_done, hipEventDisableTiming));
    STAMPS_HIP_CHECK(hipMemsetAsync(h->d_logs, 0, 2 * S * sizeof(ccs::Log), h->stream));
    STAMPS_HIP_CHECK(hipMemsetAsync(h->d_missing, 0, S * sizeof(ull), h->stream));
    STAMPS_HIP_CHECK(hipMemsetAsync(h->d_rings, 0, S * h->capacity * sizeof(uint64_t), h->stream));
    return CC_OK;
}

// h_stage, free to be written
int take_stage(cc_firing_stamps* h)
{
    if (h->stage_pending)
    {
        STAMPS_HIP_CHECK(hipEventSynchronize(h->stage_done));
        h->stage_pending = false;
    }
    return CC_OK;
}

int upload_stage(cc_firing_stamps* h, size_t bytes)
{
    STAMPS_HIP_CHECK(hipMemcpyAsync(h->d_stage, h->h_stage, bytes, hipMemcpyHostToDevice, h->stream));
    STAMPS_HIP_CHECK(hipEventRecord(h->stage_done, h->stream));
    h->stage_pending = true;
    return CC_OK;
}

int no_such_stream(const cc_firing_stamps* h, const char* who, int stream)
{
    return fail(CC_ERR_INVALID_ARGUMENT,
                std::string(who) + ": no such stream " + std::to_string(stream) + " (the log has " + std::to_string(h->num_streams) + ")");
}

} // namespace

extern "C" {

const char* cc_firing_stamps_last_error(void)
{
    return g_stamps_error.c_str();
}

// ---- host twins -----------------------------------------------------------------------------------------------------------------------------------

int64_t cc_stamps_round_capacity(int64_t capacity)
{
    if (capacity < 1 || (uint64_t) capacity > MAX_CAPACITY)
        return 0;
    int64_t c = 1;
    while (c < capacity)
        c <<= 1;
    return c;
}

int cc_stamps_host_push(cc_stamps_host_log* log, int stream, int64_t n, const uint64_t* stamps, int repeat)
{
    if (const char* bad = bad_host_log(log))
        return fail(CC_ERR_INVALID_ARGUMENT, std::string("cc_stamps_host_push: ") + bad);
    if (stream < -1 || stream >= log->num_streams)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_stamps_host_push: no such stream " + std::to_string(stream));
    if (n < 1 || repeat < 1 || !stamps || n > log->capacity / repeat)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_stamps_host_push: stamps, n >= 1, repeat >= 1 and n * repeat <= capacity are required");
    for (int s = stream < 0 ? 0 : stream; s < (stream < 0 ? log->num_streams : stream + 1); s++)
    {
        const uint64_t* src = stamps + (stream < 0 ? (size_t) s * (size_t) n : 0);
        uint64_t* ring = log->rings + (size_t) s * (size_t) log->capacity;
        for (int64_t t = 0; t < n * repeat; t++)
            ring[(log->heads[s] + (uint64_t) t) & (uint64_t) (log->capacity - 1)] = src[t / repeat];
        log->heads[s] += (uint64_t) (n * repeat);
    }
    return CC_OK;
}

int cc_stamps_host_resolve(const cc_stamps_host_log* log, int stream, int64_t n, const uint32_t* firings, uint64_t* stamps, uint8_t* missing)
{
    if (const char* bad = bad_host_log(log))
        return fail(CC_ERR_INVALID_ARGUMENT, std::string("cc_stamps_host_resolve: ") + bad);
    if (stream < 0 || stream >= log->num_streams)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_stamps_host_resolve: no such stream " + std::to_string(stream));
    if (n < 0 || (n > 0 && (!firings || !stamps)))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_stamps_host_resolve: firings and stamps are required");
    for (int64_t i = 0; i < n; i++)
    {
        bool miss;
        stamps[i] = host_resolve(log, stream, firings[i], &miss);
        if (missing)
            missing[i] = miss ? 1 : 0;
    }
    return CC_OK;
}

int cc_stamps_host_sec_nsec(int64_t n, const uint64_t* stamps, uint32_t* out)
{
    if (n < 0 || (n > 0 && (!stamps || !out)))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_stamps_host_sec_nsec: stamps and out are required");
    for (int64_t i = 0; i < n; i++)
        ccs::sec_nsec(stamps[i], out + 2 * i, out + 2 * i + 1);
    return CC_OK;
}

int cc_stamps_host_of_points(cc_stamps_host_log* log, int64_t n_records, const cc_take_point* records, const cc_take_stream* table,
                             uint64_t* stamps, uint32_t* sec_nsec)
{
    if (const char* bad = bad_host_log(log))
        return fail(CC_ERR_INVALID_ARGUMENT, std::string("cc_stamps_host_of_points: ") + bad);
    if (n_records < 0 || !table || (n_records > 0 && (!records || !stamps)))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_stamps_host_of_points: records, table and stamps are required");
    for (int64_t i = 0; i < n_records; i++)
    {
        const int s = ccs::slice_of(log->num_streams, i, [&](int k) { return table[k].first_record; });
        uint64_t stamp = 0;
        if (s >= 0)
        {
            bool miss;
            stamp = host_resolve(log, s, records[i].source_firing, &miss);
            log->missing[s] += miss ? 1 : 0;
        }
        stamps[i] = stamp;
        if (sec_nsec)
            ccs::sec_nsec(stamp, sec_nsec + 2 * i, sec_nsec + 2 * i + 1);
    }
    return CC_OK;
}

int cc_stamps_host_of_columns(cc_stamps_host_log* log, int64_t n_records, const cc_take_point* records, const cc_take_stream* table,
                              uint64_t* column_stamps, uint64_t* stream_stamps)
{
    if (const char* bad = bad_host_log(log))
        return fail(CC_ERR_INVALID_ARGUMENT, std::string("cc_stamps_host_of_columns: ") + bad);
    if (n_records < 0 || !table || (n_records > 0 && !records))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_stamps_host_of_columns: records and table are required");
    const int S = log->num_streams;
    std::vector<int64_t> offsets((size_t) S + 1, 0);
    for (int s = 0; s < S; s++)
        offsets[(size_t) s + 1] = offsets[(size_t) s] + columns_of(table[s]);
    std::vector<uint64_t> column_keys((size_t) offsets[(size_t) S], NO_STAMP), stream_keys((size_t) S, NO_STAMP);
    for (int64_t i = 0; i < n_records; i++)
    {
        const int s = ccs::slice_of(S, i, [&](int k) { return table[k].first_record; });
        if (s < 0)
            continue;
        bool miss;
        const uint64_t key = ccs::nonzero_min_key(host_resolve(log, s, records[i].source_firing, &miss));
        log->missing[s] += miss ? 1 : 0;
        if (key < stream_keys[(size_t) s])
            stream_keys[(size_t) s] = key;
        const int64_t at = offsets[(size_t) s] + (int64_t) records[i].column;
        if (at < offsets[(size_t) s + 1] && key < column_keys[(size_t) at])
            column_keys[(size_t) at] = key;
    }
    if (column_stamps)
        for (size_t c = 0; c < column_keys.size(); c++)
            column_stamps[c] = ccs::nonzero_min_from_key(column_keys[c]);
    if (stream_stamps)
        for (int s = 0; s < S; s++)
            stream_stamps[s] = ccs::nonzero_min_from_key(stream_keys[(size_t) s]);
    return CC_OK;
}

int cc_stamps_host_of_clusters(cc_stamps_host_log* log, int use_last_point, int64_t n_clusters, const cc_take_cluster* clusters,
                               int64_t n_records, const cc_take_point* records, cc_cluster_stamp* out, uint64_t* point_stamps)
{
    if (const char* bad = bad_host_log(log))
        return fail(CC_ERR_INVALID_ARGUMENT, std::string("cc_stamps_host_of_clusters: ") + bad);
    if (n_clusters < 0 || n_records < 0 || n_clusters > INT32_MAX || (n_clusters > 0 && (!clusters || !out)))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_stamps_host_of_clusters: clusters and out are required");
    if (n_records > 0 && !records)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_stamps_host_of_clusters: stamps need the records (none after CC_TAKE_CLUSTERS_DESCRIPTORS_ONLY)");
    for (int64_t c = 0; c < n_clusters; c++)
        out[c] = cc_cluster_stamp{0, NO_STAMP, 0, 0, 0};
    for (int64_t i = 0; i < n_records && n_clusters > 0; i++)
    {
        const int c = ccs::slice_of((int) n_clusters, i, [&](int k) { return clusters[k].first_record; });
        if (c < 0 || i >= clusters[c].first_record + (int64_t) clusters[c].n_points)
            continue;
        const int s = clusters[c].stream;
        bool miss = true;
        uint64_t stamp = 0;
        if (s >= 0 && s < log->num_streams)
        {
            stamp = host_resolve(log, s, records[i].source_firing, &miss);
            log->missing[s] += miss ? 1 : 0;
        }
        out[c].n_missing += miss ? 1 : 0;
        if (stamp < out[c].min_stamp)
            out[c].min_stamp = stamp;
        if (stamp > out[c].max_stamp)
            out[c].max_stamp = stamp;
        if (point_stamps)
            point_stamps[i] = stamp;
    }
    for (int64_t c = 0; c < n_clusters; c++)
    {
        if (out[c].min_stamp > out[c].max_stamp)
            out[c] = cc_cluster_stamp{0, 0, 0, 0, 0};
        else
            out[c].stamp = ccs::cluster_stamp(out[c].min_stamp, out[c].max_stamp, use_last_point != 0);
    }
    return CC_OK;
}

// ---- device ---------------------------------------------------------------------------------------------------------------------------------------

int cc_firing_stamps_create(cc_firing_stamps** out, int device, int num_streams, int64_t capacity, void* hip_stream)
{
    if (!out)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_create: null output handle");
    *out = nullptr;
    if (num_streams <= 0 || num_streams > 65535)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_create: 1 to 65535 streams (the grid's second dimension)");
    const int64_t rounded = cc_stamps_round_capacity(capacity);
    if (rounded == 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_create: capacity must be 1 to 2^31 firings, not " + std::to_string(capacity));
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(CC_ERR_NO_DEVICE, "cc_firing_stamps_create: no gfx950 device (there is no CPU variant of this path)");
    cc_firing_stamps* h = new cc_firing_stamps;
    h->device = device;
    h->num_streams = num_streams;
    h->capacity = (uint64_t) rounded;
    const int rc = create(h, hip_stream);
    if (rc != CC_OK)
    {
        release(h);
        return rc;
    }
    *out = h;
    return CC_OK;
}

void cc_firing_stamps_destroy(cc_firing_stamps* h)
{
    if (h)
        release(h);
}

void* cc_firing_stamps_hip_stream(cc_firing_stamps* h)
{
    return h ? (void*) h->stream : nullptr;
}

int cc_firing_stamps_sync(cc_firing_stamps* h)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_sync: null handle");
    STAMPS_HIP_CHECK(hipSetDevice(h->device));
    STAMPS_HIP_CHECK(hipStreamSynchronize(h->stream));
    return CC_OK;
}

int64_t cc_firing_stamps_capacity(cc_firing_stamps* h)
{
    return h ? (int64_t) h->capacity : 0;
}

int cc_firing_stamps_push(cc_firing_stamps* h, int64_t n, const uint64_t* d_stamps, int repeat)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_push: null handle");
    if (n < 1 || repeat < 1)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_push: n and repeat must be positive");
    if ((uint64_t) n > h->capacity / (uint64_t) repeat)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_push: " + std::to_string(n) + " stamps x " + std::to_string(repeat) +
                                                 " exceed the capacity of " + std::to_string(h->capacity) + " firings");
    if (!d_stamps || (uintptr_t) d_stamps % 8 != 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_push: d_stamps is required, 8-byte aligned");
    STAMPS_HIP_CHECK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_push, dim3(blocks_for(n * repeat), (unsigned) h->num_streams), dim3(BLOCK), 0, h->stream, h->cur(), h->next(), h->d_rings,
                       h->capacity, d_stamps, n, repeat, -1);
    STAMPS_HIP_CHECK(hipGetLastError());
    h->gen++;
    return CC_OK;
}

int cc_firing_stamps_push_host(cc_firing_stamps* h, int stream, int64_t n, const uint64_t* stamps)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_push_host: null handle");
    if (stream < 0 || stream >= h->num_streams)
        return no_such_stream(h, "cc_firing_stamps_push_host", stream);
    if (n < 1 || (uint64_t) n > h->capacity)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_push_host: " + std::to_string(n) + " stamps not in 1..capacity (" +
                                                 std::to_string(h->capacity) + ")");
    if (!stamps)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_push_host: stamps is required");
    STAMPS_HIP_CHECK(hipSetDevice(h->device));
    int rc = take_stage(h);
    if (rc != CC_OK)
        return rc;
    std::memcpy(h->h_stage, stamps, (size_t) n * sizeof(uint64_t));
    rc = upload_stage(h, (size_t) n * sizeof(uint64_t));
    if (rc != CC_OK)
        return rc;
    hipLaunchKernelGGL(k_push, dim3(blocks_for(n), (unsigned) h->num_streams), dim3(BLOCK), 0, h->stream, h->cur(), h->next(), h->d_rings,
                       h->capacity, (const uint64_t*) h->d_stage, n, 1, stream);
    STAMPS_HIP_CHECK(hipGetLastError());
    h->gen++;
    return CC_OK;
}

int cc_firing_stamps_seek(cc_firing_stamps* h, int stream, uint64_t next_firing)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_seek: null handle");
    if (stream < 0 || stream >= h->num_streams)
        return no_such_stream(h, "cc_firing_stamps_seek", stream);
    STAMPS_HIP_CHECK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_seek, dim3(blocks_for(h->num_streams)), dim3(BLOCK), 0, h->stream, h->cur(), h->next(), h->num_streams, stream,
                       next_firing);
    STAMPS_HIP_CHECK(hipGetLastError());
    h->gen++;
    return CC_OK;
}

int cc_firing_stamps_reset_streams(cc_firing_stamps* h, int n, const int* streams)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_reset_streams: null handle");
    if (n < 0 || (n > 0 && !streams))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_reset_streams: n >= 0 and a list of streams are required");
    for (int i = 0; i < n; i++)
        if (streams[i] < 0 || streams[i] >= h->num_streams)
            return no_such_stream(h, "cc_firing_stamps_reset_streams", streams[i]);
    if (n == 0)
        return CC_OK;
    STAMPS_HIP_CHECK(hipSetDevice(h->device));
    int rc = take_stage(h);
    if (rc != CC_OK)
        return rc;
    std::memset(h->h_stage, 0, (size_t) h->num_streams);
    for (int i = 0; i < n; i++)
        h->h_stage[streams[i]] = 1;
    rc = upload_stage(h, (size_t) h->num_streams);
    if (rc != CC_OK)
        return rc;
    hipLaunchKernelGGL(k_reset, dim3(blocks_for(h->num_streams)), dim3(BLOCK), 0, h->stream, h->cur(), h->next(), h->d_missing, h->num_streams,
                       (const uint8_t*) h->d_stage);
    STAMPS_HIP_CHECK(hipGetLastError());
    h->gen++;
    return CC_OK;
}

int cc_firing_stamps_counters(cc_firing_stamps* h, int stream, uint64_t* head, uint64_t* missing)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_counters: null handle");
    if (stream < 0 || stream >= h->num_streams)
        return no_such_stream(h, "cc_firing_stamps_counters", stream);
    STAMPS_HIP_CHECK(hipSetDevice(h->device));
    ccs::Log log;
    ull lost;
    STAMPS_HIP_CHECK(hipMemcpyAsync(&log, h->cur() + stream, sizeof(log), hipMemcpyDeviceToHost, h->stream));
    STAMPS_HIP_CHECK(hipMemcpyAsync(&lost, h->d_missing + stream, sizeof(lost), hipMemcpyDeviceToHost, h->stream));
    STAMPS_HIP_CHECK(hipStreamSynchronize(h->stream));
    if (head)
        *head = log.head;
    if (missing)
        *missing = lost;
    return CC_OK;
}

int cc_firing_stamps_of_points(cc_firing_stamps* h, int64_t n_records, const cc_take_point* d_records, const cc_take_stream* d_table,
                               uint64_t* d_stamps, uint32_t* d_sec_nsec)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_points: null handle");
    if (n_records < 0 || n_records > (int64_t) INT32_MAX * BLOCK)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_points: n_records out of range");
    if (!d_table)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_points: d_table, the device table of the take, is required");
    if (n_records == 0)
        return CC_OK;
    if (!d_records || !d_stamps)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_points: d_records and d_stamps are required");
    if ((uintptr_t) d_records % 16 != 0 || (uintptr_t) d_table % 8 != 0 || (uintptr_t) d_stamps % 8 != 0 || (uintptr_t) d_sec_nsec % 8 != 0)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_points: misaligned buffer (d_records 16 B, d_table, d_stamps, d_sec_nsec 8 B)");
    STAMPS_HIP_CHECK(hipSetDevice(h->device));
    auto kernel = h->num_streams <= LDS_STREAMS ? k_of_points<true> : k_of_points<false>;
    hipLaunchKernelGGL(kernel, dim3(blocks_for(n_records)), dim3(BLOCK), 0, h->stream, h->cur(), (const uint64_t*) h->d_rings, h->capacity,
                       h->d_missing, h->num_streams, n_records, d_records, d_table, d_stamps, (uint2*) d_sec_nsec);
    STAMPS_HIP_CHECK(hipGetLastError());
    return CC_OK;
}

int cc_firing_stamps_of_columns(cc_firing_stamps* h, int64_t n_records, const cc_take_point* d_records, const cc_take_stream* d_table,
                                const cc_take_stream* h_table, uint64_t* d_column_stamps, uint64_t* d_stream_stamps)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_columns: null handle");
    if (n_records < 0 || n_records > (int64_t) INT32_MAX * BLOCK)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_columns: n_records out of range");
    if (!d_table)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_columns: d_table, the device table of the take, is required");
    if (n_records > 0 && !d_records)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_columns: d_records is required");
    if ((uintptr_t) d_records % 16 != 0 || (uintptr_t) d_table % 8 != 0 || (uintptr_t) d_column_stamps % 8 != 0 ||
        (uintptr_t) d_stream_stamps % 8 != 0)
        return fail(CC_ERR_INVALID_ARGUMENT,
                    "cc_firing_stamps_of_columns: misaligned buffer (d_records 16 B, d_table, d_column_stamps, d_stream_stamps 8 B)");
    STAMPS_HIP_CHECK(hipSetDevice(h->device));
    const int S = h->num_streams;
    if (!h_table)
    {
        h->table.resize((size_t) S);
        STAMPS_HIP_CHECK(hipMemcpyAsync(h->table.data(), d_table, (size_t) S * sizeof(cc_take_stream), hipMemcpyDeviceToHost, h->stream));
        STAMPS_HIP_CHECK(hipStreamSynchronize(h->stream));
        h_table = h->table.data();
    }
    int64_t n_columns = 0;
    for (int s = 0; s < S; s++)
        n_columns += columns_of(h_table[s]);
    if (n_columns > (int64_t) INT32_MAX * BLOCK)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_columns: the table's column ranges are out of range");
    if (!d_column_stamps)
        n_columns = 0;
    if (n_columns == 0 && !d_stream_stamps)
        return CC_OK;
    // the outputs hold keys (stamp - 1) while the minimum is taken: 2^64 - 1 is the identity and finishes as stamp 0
    if (n_columns > 0)
        STAMPS_HIP_CHECK(hipMemsetAsync(d_column_stamps, 0xFF, (size_t) n_columns * sizeof(uint64_t), h->stream));
    if (d_stream_stamps)
        STAMPS_HIP_CHECK(hipMemsetAsync(d_stream_stamps, 0xFF, (size_t) S * sizeof(uint64_t), h->stream));
    if (n_records > 0)
    {
        hipLaunchKernelGGL(k_column_offsets, dim3(1), dim3(BLOCK), 0, h->stream, d_table, S, h->d_offsets);
        auto kernel = S <= LDS_STREAMS ? k_of_columns<true> : k_of_columns<false>;
        hipLaunchKernelGGL(kernel, dim3(blocks_for(n_records)), dim3(BLOCK), 0, h->stream, h->cur(), (const uint64_t*) h->d_rings, h->capacity,
                           h->d_missing, S, n_records, d_records, d_table, (const int64_t*) h->d_offsets, n_columns,
                           (ull*) (n_columns > 0 ? d_column_stamps : nullptr), (ull*) d_stream_stamps);
    }
    if (n_columns > 0)
        hipLaunchKernelGGL(k_keys_to_stamps, dim3(blocks_for(n_columns)), dim3(BLOCK), 0, h->stream, d_column_stamps, n_columns);
    if (d_stream_stamps)
        hipLaunchKernelGGL(k_keys_to_stamps, dim3(blocks_for(S)), dim3(BLOCK), 0, h->stream, d_stream_stamps, (int64_t) S);
    STAMPS_HIP_CHECK(hipGetLastError());
    return CC_OK;
}

int cc_firing_stamps_of_clusters(cc_firing_stamps* h, int use_last_point, int64_t n_clusters, const cc_take_cluster* d_clusters,
                                 int64_t n_records, const cc_take_point* d_records, cc_cluster_stamp* d_out, uint64_t* d_point_stamps)
{
    if (!h)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_clusters: null handle");
    if (n_clusters < 0 || n_clusters > INT32_MAX || n_records < 0 || n_records > (int64_t) INT32_MAX * BLOCK)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_clusters: n_clusters or n_records out of range");
    if (n_records > 0 && !d_records)
        return fail(CC_ERR_INVALID_ARGUMENT,
                    "cc_firing_stamps_of_clusters: stamps need the records (there are none after CC_TAKE_CLUSTERS_DESCRIPTORS_ONLY)");
    if (n_clusters == 0)
        return CC_OK;
    if (!d_clusters || !d_out)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_firing_stamps_of_clusters: d_clusters and d_out are required");
    if ((uintptr_t) d_records % 16 != 0 || (uintptr_t) d_clusters % 16 != 0 || (uintptr_t) d_out % 16 != 0 || (uintptr_t) d_point_stamps % 8 != 0)
        return fail(CC_ERR_INVALID_ARGUMENT,
                    "cc_firing_stamps_of_clusters: misaligned buffer (d_records, d_clusters, d_out 16 B, d_point_stamps 8 B)");
    STAMPS_HIP_CHECK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_clusters_init, dim3(blocks_for(n_clusters)), dim3(BLOCK), 0, h->stream, d_out, n_clusters);
    if (n_records > 0)
        hipLaunchKernelGGL(k_of_clusters, dim3(blocks_for(n_records)), dim3(BLOCK), 0, h->stream, h->cur(), (const uint64_t*) h->d_rings,
                           h->capacity, h->d_missing, h->num_streams, n_clusters, d_clusters, n_records, d_records, d_out, d_point_stamps);
    hipLaunchKernelGGL(k_clusters_finish, dim3(blocks_for(n_clusters)), dim3(BLOCK), 0, h->stream, d_out, n_clusters, use_last_point);
    STAMPS_HIP_CHECK(hipGetLastError());
    return CC_OK;
}

} // extern "C"
