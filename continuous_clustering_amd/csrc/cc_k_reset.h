// cc_k_reset.h — k_reset_streams: reset(num_rows) (cc.cpp:11-64) for a LIST of streams of a multi-stream engine in one launch
// (cc_engine_reset_streams).
// (part of cc_kernels.h: included there, in order, inside namespace cck)
//
// What the engine's whole reset does with nine hipMemsetAsync over whole planes and one copy of every stream's StreamState, this kernel does for the
// listed streams' slices only: the same planes, the same fill bytes, the same StreamState (built on the host by the function the whole reset
// uses), and the streams' hand-over cursors. Every other stream is live: the slice of stream s of a plane is the bytes [s * bytes, (s + 1) * bytes)
// and nothing outside it is written. A slice does not start on 16 bytes in general (1- and 2-byte planes, odd cell counts): fill_slice writes
// the bytes up to the first 16-byte boundary and behind the last one singly and the aligned middle as 16-byte stores. Plain vector stores only;
// the engine has drained every chain before the launch and synchronises behind it, so nothing reads or writes these bytes meanwhile. A stream
// listed twice is written twice with the same values.
#pragma once

constexpr int RESET_PLANES = 9;    // dist, gtag, id, ground, debug, ignored, root, tab_acc, sl_ctl (cc_engine.hip: reset_state)
constexpr int RESET_THREADS = 256;
constexpr unsigned long long RESET_CHUNK_BYTES = 16384; // of the longest slice per block, while the launch stays below RESET_MAX_BLOCKS blocks
constexpr int RESET_MAX_BLOCKS = 2048;
static_assert(sizeof(StreamState) % sizeof(unsigned long long) == 0 && alignof(StreamState) == alignof(unsigned long long), "the state is copied in 8-byte words");

struct ResetFill
{
    char* plane;              // first byte of the plane (stream 0)
    unsigned long long bytes; // of one stream's slice
    unsigned value;           // the byte every byte of the slice becomes (hipMemset's value)
    unsigned pad;
};

struct ResetJob
{
    ResetFill fill[RESET_PLANES];
    StreamState fresh;       // a stream as reset leaves it
    StreamState* states;
    long long* take_cursor;  // [2 stages][streams], or null: no take_points yet
    long long* tc_cursor;    // [streams][2], or null: no take_clusters yet
    int num_streams;
    int pad;
};

// bytes [p, p + bytes) = value, by block `chunk` of `chunks` blocks of RESET_THREADS threads
__device__ __forceinline__ void fill_slice(char* p, const unsigned long long bytes, const unsigned value, const unsigned chunk, const unsigned chunks)
{
    const unsigned long long to_boundary = (16ull - ((unsigned long long) p & 15ull)) & 15ull;
    const unsigned long long head = to_boundary < bytes ? to_boundary : bytes; // bytes in front of the first 16-byte boundary inside the slice
    const unsigned long long words = (bytes - head) >> 4;                       // whole 16-byte words behind it
    const unsigned long long tail = bytes - head - (words << 4);                // bytes behind the last of them: head + 16 * words + tail = bytes
    const unsigned w = (value & 0xffu) * 0x01010101u;
    const uint4 v = make_uint4(w, w, w, w);
    uint4* mid = (uint4*) (p + head);
    for (unsigned long long i = (unsigned long long) chunk * RESET_THREADS + threadIdx.x; i < words; i += (unsigned long long) chunks * RESET_THREADS)
        mid[i] = v;
    if (chunk == 0 && threadIdx.x < head)
        p[threadIdx.x] = (char) value;
    if (chunk == chunks - 1 && threadIdx.x < tail)
        p[head + (words << 4) + threadIdx.x] = (char) value;
}

// =====================================================================================================
// k_reset_streams — grid (chunks, listed streams), RESET_THREADS threads. Block (c, j) fills its share of every slice of stream list[j]; block
// (0, j) also stores the stream's state and cursors. The host sizes the grid from the list and the longest slice, never from the number of
// streams of the engine.
// =====================================================================================================
__global__ __launch_bounds__(RESET_THREADS) void k_reset_streams(const ResetJob job, const int* __restrict__ list)
{
    const int s = list[blockIdx.y];
    if (s < 0 || s >= job.num_streams)
        return; // (never: the host has checked the list)
    for (int k = 0; k < RESET_PLANES; k++)
        fill_slice(job.fill[k].plane + (unsigned long long) s * job.fill[k].bytes, job.fill[k].bytes, job.fill[k].value, blockIdx.x, gridDim.x);
    if (blockIdx.x != 0)
        return;
    const unsigned long long* src = (const unsigned long long*) &job.fresh;
    unsigned long long* dst = (unsigned long long*) &job.states[s];
    for (unsigned i = threadIdx.x; i < sizeof(StreamState) / sizeof(unsigned long long); i += RESET_THREADS)
        dst[i] = src[i];
    if (threadIdx.x < 2)
    {
        if (job.take_cursor)
            job.take_cursor[(size_t) threadIdx.x * job.num_streams + s] = 0;
        if (job.tc_cursor)
            job.tc_cursor[2 * (size_t) s + threadIdx.x] = 0;
    }
}
