// cc_ouster.hip — Ouster lidar packets (LEGACY, RNG19_RFL8_SIG16_NIR16 and its _DUAL UDP profile) -> engine firings on gfx950
// (include/cc_ouster.h, include/cc_ouster_profiles.h).
//
// One kernel, k_ouster_decode, one 256-thread workgroup per (packet, stream). Pure streaming:
//   1. the packet (header + C columns + footer, 6464 B for a LEGACY OS-32) is staged into LDS with 16-byte loads (pixels sit at a 12-byte
//      stride, or at 16 bytes from a 4-byte-aligned base, so per-lane loads straight from HBM would be dword loads at odd alignment);
//   2. wave 0 reads the C column headers from LDS (status, measurement id) and decides which columns become placeholders;
//   3. every lane then writes 16 contiguous bytes of the packet's output regions: C*H*12 B of xyz (the C firings of a packet are adjacent
//      in [S][n][H][3]), C*H B of intensity, C*96 B of replicated poses. The LUT rows a column reads ([m_id][row][3], 12 H bytes) are
//      contiguous too and are read as float4; the whole LUT (W*H*24 B, 786 KB for 32 x 1024) stays in L2.
// HBM bytes per packet: written C*(13 H + 96 + 4) for every profile (14.5 B per cell for 64 x 16); read, with the 96 B packet pose,
//   LEGACY                       C*(20 + 12 H) + 96        12.4 B per cell for 64 x 16
//   RNG19_RFL8_SIG16_NIR16       C*(12 + 12 H) + 64 + 96   12.3 B per cell
//   RNG19_RFL8_SIG16_NIR16_DUAL  C*(12 + 16 H) + 64 + 96   16.3 B per cell (the second return is staged with its packet and never read)
//
// The layout lives in one descriptor per profile (PacketLayout, LAYOUTS) that the kernel takes by value: its fields are kernel arguments,
// uniform over the grid, so no lane branches on the profile. Device code is built with -ffp-contract=off and spells the cartesianT
// arithmetic with __fmul_rn / __fadd_rn anyway: x = (float) r * d + o, two roundings.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cc_hip.h"
#include "../../include/cc_ouster.h"
#include "../../include/cc_ouster_profiles.h"

namespace
{

thread_local std::string g_ouster_error;

int fail(int code, const std::string& what)
{
    g_ouster_error = what;
    return code;
}

#define OUSTER_HIP_CHECK(expr)                                                                         \
    do                                                                                                 \
    {                                                                                                  \
        hipError_t err__ = (expr);                                                                     \
        if (err__ != hipSuccess)                                                                       \
            return fail(CC_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(err__));             \
    } while (0)

// Byte layout of a packet of one UDP profile (column offsets are within the column; H = pixels per column).
struct PacketLayout
{
    int packet_header_bytes; // before the first column; as many bytes follow the last column (neither is ever looked at)
    int header_bytes;        // column header before the first pixel
    int pixel_stride;        // bytes per pixel
    int range_offset;        // u32 range within a pixel
    uint32_t range_mask;     // range bits (millimetres)
    int signal_offset;       // u16 signal within a pixel
    int measurement_offset;  // u16 measurement id within the header
    int status_offset;       // status within the column; -1: behind the last pixel (header_bytes + pixel_stride * H)
    int status_bytes;        // 4: u32 status, 2: u16 status
    int trailer_bytes;       // bytes of the column behind the last pixel
    uint32_t status_valid;   // column is valid iff status & status_valid (ouster_input.hpp:120-125)
};

// Restated from the SDK's packet_format and field tables: UNPINNED, all three (include/cc_ouster_profiles.h has the table). LEGACY is the
// profile of the reference's calibrations/touareg_os32_*.json. Indexed by the CC_OUSTER_PROFILE_* enum.
constexpr PacketLayout LAYOUTS[] = {
    {0, 16, 12, 0, 0x000FFFFFu, 6, 8, -1, 4, 4, 0x1u},  // LEGACY
    {32, 12, 12, 0, 0x0007FFFFu, 6, 8, 10, 2, 0, 0x1u}, // RNG19_RFL8_SIG16_NIR16
    {32, 12, 16, 0, 0x0007FFFFu, 8, 8, 10, 2, 0, 0x1u}, // RNG19_RFL8_SIG16_NIR16_DUAL (first return only, as the reference)
};
constexpr int NUM_PROFILES = sizeof(LAYOUTS) / sizeof(LAYOUTS[0]);

constexpr int BLOCK = 256;
constexpr int MAX_ROWS = 128;
constexpr int MAX_COLUMNS_PER_PACKET = 64; // wave 0 holds one column header per lane
constexpr int64_t MAX_LDS_BYTES = 65536;   // of one workgroup: the staged packet and s_mid

int column_bytes(const PacketLayout& L, int H)
{
    return L.header_bytes + L.pixel_stride * H + L.trailer_bytes;
}

int64_t packet_bytes_of(const PacketLayout& L, int H, int C)
{
    return 2 * (int64_t) L.packet_header_bytes + (int64_t) C * column_bytes(L, H);
}

// The layout with status_offset resolved for H rows (what the kernel takes).
PacketLayout resolved(PacketLayout L, int H)
{
    if (L.status_offset < 0)
        L.status_offset = L.header_bytes + L.pixel_stride * H;
    return L;
}

struct StreamLut
{
    const float* direction; // [W][H][3]
    const float* offset;    // [W][H][3]
    int columns;            // W
    int pad;
};

enum
{
    CNT_INVALID = 0,
    CNT_BAD_MID = 1,
    CNT_SKIPPED = 2,
    NUM_COUNTERS = 3
};

struct DecodeArgs
{
    const unsigned char* packets;  // [S][P][packet_bytes]
    const double* packet_poses;    // [S][P][12] or null
    const unsigned char* skip;     // [S][P] or null
    float* xyz;                    // [S][P*C][H][3]
    unsigned char* intensity;      // [S][P*C][H]
    double* poses;                 // [S][P*C][12]
    int* measurement_id;           // [S][P*C] or null
    const StreamLut* luts;         // [S]
    unsigned long long* counters;  // [S][NUM_COUNTERS]
    PacketLayout L;
    int H, C, n_packets, col_bytes, packet_bytes, vec16;
};

__device__ __forceinline__ uint32_t lds_u32(const unsigned char* p)
{
    return *(const uint32_t*) p;
}

__device__ __forceinline__ uint32_t lds_u16(const unsigned char* p)
{
    return *(const unsigned short*) p;
}

__global__ __launch_bounds__(BLOCK) void k_ouster_decode(DecodeArgs a)
{
    extern __shared__ uint4 s_pkt[];
    __shared__ int s_mid[MAX_COLUMNS_PER_PACKET]; // LUT column of each packet column, -1 = placeholder
    const int p = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const int H = a.H, C = a.C, H3 = 3 * H;
    const PacketLayout& L = a.L;
    const size_t pk = (size_t) s * a.n_packets + p;
    const bool skipped = a.skip && a.skip[pk];
    const unsigned char* sb = (const unsigned char*) s_pkt + L.packet_header_bytes; // column 0

    // 1. stage the packet
    if (!skipped)
    {
        const unsigned char* src = a.packets + pk * (size_t) a.packet_bytes;
        if (a.vec16)
            for (int i = tid; i < a.packet_bytes / 16; i += BLOCK)
                s_pkt[i] = ((const uint4*) src)[i];
        else
            for (int i = tid; i < a.packet_bytes / 4; i += BLOCK)
                ((uint32_t*) s_pkt)[i] = ((const uint32_t*) src)[i];
    }
    __syncthreads();

    // 2. column headers (wave 0, one column per lane)
    if (tid < 64)
    {
        const StreamLut lut = a.luts[s];
        int m = -1;
        bool invalid = false, bad_mid = false;
        if (tid < C && !skipped)
        {
            const unsigned char* col = sb + tid * a.col_bytes;
            const uint32_t status = L.status_bytes == 4 ? lds_u32(col + L.status_offset) : lds_u16(col + L.status_offset);
            const int mid = (int) lds_u16(col + L.measurement_offset);
            invalid = !(status & L.status_valid);
            bad_mid = !invalid && mid >= lut.columns; // the reference would read its LUT out of bounds
            m = invalid || bad_mid ? -1 : mid;
        }
        if (tid < C)
            s_mid[tid] = m;
        const unsigned long long n_invalid = __popcll(__ballot(invalid)), n_bad = __popcll(__ballot(bad_mid));
        if (tid == 0)
        {
            unsigned long long* cnt = a.counters + (size_t) s * NUM_COUNTERS;
            if (n_invalid)
                atomicAdd(cnt + CNT_INVALID, n_invalid);
            if (n_bad)
                atomicAdd(cnt + CNT_BAD_MID, n_bad);
            if (skipped)
                atomicAdd(cnt + CNT_SKIPPED, 1ull);
        }
    }
    __syncthreads();

    const size_t firing0 = (size_t) s * a.n_packets * C + (size_t) p * C; // first output firing of this packet
    const StreamLut lut = a.luts[s];
    const float qnan = __builtin_nanf("");

    // 3a. xyz: float4 i of the packet's C*H*3 floats. H % 4 == 0, so a float4 never straddles two columns and the LUT float4 is aligned.
    float4* xyz = (float4*) (a.xyz + firing0 * H3);
    for (int i = tid; i < C * H3 / 4; i += BLOCK)
    {
        const int e = 4 * i, k = e / H3, w = e - k * H3;
        const int m = s_mid[k];
        float v[4] = {qnan, qnan, qnan, qnan};
        if (m >= 0)
        {
            const float4 d = *(const float4*) (lut.direction + (size_t) m * H3 + w);
            const float4 o = *(const float4*) (lut.offset + (size_t) m * H3 + w);
            const float dv[4] = {d.x, d.y, d.z, d.w}, ov[4] = {o.x, o.y, o.z, o.w};
            const unsigned char* col = sb + k * a.col_bytes + L.header_bytes + L.range_offset;
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                const int row = (w + j) / 3;
                const uint32_t r = lds_u32(col + row * L.pixel_stride) & L.range_mask;
                const float x = __fadd_rn(__fmul_rn((float) r, dv[j]), ov[j]); // SDK cartesianT
                v[j] = r > 0 ? x : qnan;
            }
        }
        xyz[i] = make_float4(v[0], v[1], v[2], v[3]);
    }

    // 3b. intensity: 4 cells (same column) per lane. static_cast<uint8_t>(std::min(1.f, signal / 1000.f) * 255) (ouster_input.hpp:155)
    uint32_t* inten = (uint32_t*) (a.intensity + firing0 * H);
    for (int i = tid; i < C * H / 4; i += BLOCK)
    {
        const int c0 = 4 * i, k = c0 / H, row0 = c0 - k * H;
        uint32_t packed = 0;
        if (s_mid[k] >= 0)
        {
            const unsigned char* px = sb + k * a.col_bytes + L.header_bytes + row0 * L.pixel_stride;
#pragma unroll
            for (int j = 0; j < 4; j++)
            {
                const unsigned char* q = px + j * L.pixel_stride;
                if (lds_u32(q + L.range_offset) & L.range_mask)
                {
                    const float f = __fmul_rn(fminf(1.f, __fdiv_rn((float) lds_u16(q + L.signal_offset), 1000.f)), 255.f);
                    packed |= ((uint32_t) f & 0xFFu) << (8 * j);
                }
            }
        }
        inten[i] = packed;
    }

    // 3c. poses: the packet's pose replicated to its C firings (ouster_input.hpp:111), 16 B per lane
    if (a.packet_poses)
    {
        const double2* src = (const double2*) (a.packet_poses + pk * 12);
        double2* dst = (double2*) (a.poses + firing0 * 12);
        for (int i = tid; i < 6 * C; i += BLOCK)
            dst[i] = src[i % 6];
    }
    if (a.measurement_id && tid < C)
        a.measurement_id[firing0 + tid] = s_mid[tid];
}

struct LutEntry
{
    int columns = 0;
    std::vector<float> host; // direction then offset, [W][H][3] each
    float* d = nullptr;
    int refs = 0;
};

} // namespace

struct cc_ouster
{
    int device = 0;
    int num_streams = 0;
    int rows = 0;
    int columns_per_packet = 0;
    int max_packets = 0;
    int packet_bytes = 0;
    int profile = CC_OUSTER_PROFILE_LEGACY;
    PacketLayout layout = LAYOUTS[CC_OUSTER_PROFILE_LEGACY]; // resolved for `rows`
    hipStream_t stream = nullptr;
    bool own_stream = false;
    StreamLut* d_luts = nullptr;              // [S]
    unsigned long long* d_counters = nullptr; // [S][NUM_COUNTERS]
    std::vector<LutEntry> entries;
    std::vector<int> stream_entry; // index into entries, -1 = no LUT yet
};

extern "C" {

const char* cc_ouster_last_error(void)
{
    return g_ouster_error.c_str();
}

int64_t cc_ouster_packet_bytes(int rows, int columns_per_packet)
{
    if (rows < 1 || columns_per_packet < 1)
        return 0;
    return packet_bytes_of(LAYOUTS[CC_OUSTER_PROFILE_LEGACY], rows, columns_per_packet);
}

int64_t cc_ouster_profile_packet_bytes(int profile, int rows, int columns_per_packet)
{
    if (profile < 0 || profile >= NUM_PROFILES || rows < 1 || columns_per_packet < 1)
        return 0;
    return packet_bytes_of(LAYOUTS[profile], rows, columns_per_packet);
}

int cc_ouster_profile_from_name(const char* udp_profile_lidar)
{
    if (!udp_profile_lidar)
        return -1;
    const std::string n = udp_profile_lidar;
    if (n == "LEGACY")
        return CC_OUSTER_PROFILE_LEGACY;
    if (n == "RNG19_RFL8_SIG16_NIR16")
        return CC_OUSTER_PROFILE_RNG19_RFL8_SIG16_NIR16;
    if (n == "RNG19_RFL8_SIG16_NIR16_DUAL")
        return CC_OUSTER_PROFILE_RNG19_RFL8_SIG16_NIR16_DUAL;
    if (n == "RNG15_RFL8_NIR8" || n == "FUSA_RNG15_RFL8_NIR8_DUAL")
        return -2; // no SIGNAL field: the reference's ls.field(SIGNAL) cannot run on it
    return -1;
}

int cc_ouster_profile_of(cc_ouster* o)
{
    return o ? o->profile : -1;
}

// cc_ouster_create (check_lds false: it has always left a packet beyond the LDS to the launch) and cc_ouster_create_profile.
static int create_decoder(const std::string& fn, cc_ouster** out, int device, int num_streams, int rows, int columns_per_packet, int max_packets,
                          int profile, bool check_lds, void* hip_stream)
{
    if (!out)
        return fail(CC_ERR_INVALID_ARGUMENT, fn + ": null output handle");
    *out = nullptr;
    if (profile < 0 || profile >= NUM_PROFILES)
        return fail(CC_ERR_INVALID_ARGUMENT, fn + ": no UDP profile " + std::to_string(profile) + " (CC_OUSTER_PROFILE_* of cc_ouster_profiles.h)");
    if (num_streams <= 0 || max_packets <= 0)
        return fail(CC_ERR_INVALID_ARGUMENT, fn + ": num_streams and max_packets must be positive");
    if (rows < 4 || rows > MAX_ROWS || rows % 4 != 0)
        return fail(CC_ERR_INVALID_ARGUMENT, fn + ": rows (pixels_per_column) must be a multiple of 4 in 4.." + std::to_string(MAX_ROWS));
    if (columns_per_packet < 1 || columns_per_packet > MAX_COLUMNS_PER_PACKET)
        return fail(CC_ERR_INVALID_ARGUMENT, fn + ": columns_per_packet must be in 1.." + std::to_string(MAX_COLUMNS_PER_PACKET));
    const int64_t packet_bytes = packet_bytes_of(LAYOUTS[profile], rows, columns_per_packet);
    if (check_lds && (packet_bytes + 15) / 16 * 16 + (int64_t) (MAX_COLUMNS_PER_PACKET * sizeof(int)) > MAX_LDS_BYTES)
        return fail(CC_ERR_INVALID_ARGUMENT, fn + ": a packet of " + std::to_string(packet_bytes) + " bytes (" + std::to_string(rows) + " rows x " +
                                                 std::to_string(columns_per_packet) + " columns) does not fit the 64 KB of LDS it is staged in");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
        return fail(CC_ERR_NO_DEVICE, fn + ": no gfx950 device (there is no CPU variant of this path)");
    OUSTER_HIP_CHECK(hipSetDevice(device));
    cc_ouster* o = new cc_ouster;
    o->device = device;
    o->num_streams = num_streams;
    o->rows = rows;
    o->columns_per_packet = columns_per_packet;
    o->max_packets = max_packets;
    o->packet_bytes = (int) packet_bytes;
    o->profile = profile;
    o->layout = resolved(LAYOUTS[profile], rows);
    o->stream_entry.assign(num_streams, -1);
    if (hip_stream)
        o->stream = (hipStream_t) hip_stream;
    else
    {
        OUSTER_HIP_CHECK(hipStreamCreateWithFlags(&o->stream, hipStreamNonBlocking));
        o->own_stream = true;
    }
    OUSTER_HIP_CHECK(hipMalloc(&o->d_luts, (size_t) num_streams * sizeof(StreamLut)));
    OUSTER_HIP_CHECK(hipMemset(o->d_luts, 0, (size_t) num_streams * sizeof(StreamLut)));
    OUSTER_HIP_CHECK(hipMalloc(&o->d_counters, (size_t) num_streams * NUM_COUNTERS * sizeof(unsigned long long)));
    OUSTER_HIP_CHECK(hipMemset(o->d_counters, 0, (size_t) num_streams * NUM_COUNTERS * sizeof(unsigned long long)));
    *out = o;
    return CC_OK;
}

int cc_ouster_create(cc_ouster** out, int device, int num_streams, int rows, int columns_per_packet, int max_packets, void* hip_stream)
{
    return create_decoder("cc_ouster_create", out, device, num_streams, rows, columns_per_packet, max_packets, CC_OUSTER_PROFILE_LEGACY, false,
                          hip_stream);
}

int cc_ouster_create_profile(cc_ouster** out, int device, int num_streams, int rows, int columns_per_packet, int max_packets, int profile,
                             void* hip_stream)
{
    return create_decoder("cc_ouster_create_profile", out, device, num_streams, rows, columns_per_packet, max_packets, profile, true, hip_stream);
}

void cc_ouster_destroy(cc_ouster* o)
{
    if (!o)
        return;
    (void) hipSetDevice(o->device);
    (void) hipStreamSynchronize(o->stream);
    for (LutEntry& e : o->entries)
        if (e.d)
            (void) hipFree(e.d);
    if (o->d_luts)
        (void) hipFree(o->d_luts);
    if (o->d_counters)
        (void) hipFree(o->d_counters);
    if (o->own_stream)
        (void) hipStreamDestroy(o->stream);
    delete o;
}

void* cc_ouster_hip_stream(cc_ouster* o)
{
    return o ? (void*) o->stream : nullptr;
}

int cc_ouster_sync(cc_ouster* o)
{
    if (!o)
        return fail(CC_ERR_INVALID_ARGUMENT, "null handle");
    OUSTER_HIP_CHECK(hipSetDevice(o->device));
    OUSTER_HIP_CHECK(hipStreamSynchronize(o->stream));
    return CC_OK;
}

int cc_ouster_set_lut(cc_ouster* o, int stream, int columns_per_frame, const float* direction, const float* offset)
{
    if (!o)
        return fail(CC_ERR_INVALID_ARGUMENT, "null handle");
    if (stream < -1 || stream >= o->num_streams)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_set_lut: no stream " + std::to_string(stream));
    if (columns_per_frame < 1 || columns_per_frame > 65536) // measurement_id is a u16
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_set_lut: columns_per_frame must be in 1..65536");
    if (!direction || !offset)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_set_lut: direction and offset are required");
    OUSTER_HIP_CHECK(hipSetDevice(o->device));
    const size_t n = (size_t) columns_per_frame * o->rows * 3;
    int idx = -1;
    for (size_t i = 0; i < o->entries.size() && idx < 0; i++)
    {
        const LutEntry& e = o->entries[i];
        if (e.d && e.columns == columns_per_frame && !std::memcmp(e.host.data(), direction, n * sizeof(float)) &&
            !std::memcmp(e.host.data() + n, offset, n * sizeof(float)))
            idx = (int) i;
    }
    // kernels in flight may read the table (and an entry about to be released)
    OUSTER_HIP_CHECK(hipStreamSynchronize(o->stream));
    if (idx < 0)
    {
        LutEntry e;
        e.columns = columns_per_frame;
        e.host.resize(2 * n);
        std::memcpy(e.host.data(), direction, n * sizeof(float));
        std::memcpy(e.host.data() + n, offset, n * sizeof(float));
        OUSTER_HIP_CHECK(hipMalloc(&e.d, 2 * n * sizeof(float)));
        OUSTER_HIP_CHECK(hipMemcpy(e.d, e.host.data(), 2 * n * sizeof(float), hipMemcpyHostToDevice));
        o->entries.push_back(std::move(e));
        idx = (int) o->entries.size() - 1;
    }
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? o->num_streams : stream + 1;
    for (int s = s0; s < s1; s++)
    {
        const int old = o->stream_entry[s];
        o->entries[idx].refs++;
        if (old >= 0)
            o->entries[old].refs--;
        o->stream_entry[s] = idx;
    }
    for (LutEntry& e : o->entries)
        if (e.d && e.refs == 0)
        {
            OUSTER_HIP_CHECK(hipFree(e.d));
            e.d = nullptr;
            e.host.clear();
        }
    std::vector<StreamLut> table(o->num_streams, StreamLut{nullptr, nullptr, 0, 0});
    for (int s = 0; s < o->num_streams; s++)
        if (o->stream_entry[s] >= 0)
        {
            const LutEntry& e = o->entries[o->stream_entry[s]];
            const size_t m = (size_t) e.columns * o->rows * 3;
            table[s] = StreamLut{e.d, e.d + m, e.columns, 0};
        }
    OUSTER_HIP_CHECK(hipMemcpy(o->d_luts, table.data(), table.size() * sizeof(StreamLut), hipMemcpyHostToDevice));
    return CC_OK;
}

int cc_ouster_decode(cc_ouster* o, int n_packets, const uint8_t* d_packets, const double* d_packet_poses, const uint8_t* d_skip,
                     float* d_xyz, uint8_t* d_intensity, double* d_poses, int32_t* d_measurement_id)
{
    if (!o)
        return fail(CC_ERR_INVALID_ARGUMENT, "null handle");
    if (n_packets < 0 || n_packets > o->max_packets)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_decode: n_packets " + std::to_string(n_packets) + " not in 0..max_packets (" +
                                                 std::to_string(o->max_packets) + ")");
    for (int s = 0; s < o->num_streams; s++)
        if (o->stream_entry[s] < 0)
            return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_decode: stream " + std::to_string(s) + " has no LUT (cc_ouster_set_lut)");
    if (n_packets == 0)
        return CC_OK;
    if (!d_packets || !d_xyz || !d_intensity || (d_packet_poses && !d_poses))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_decode: d_packets, d_xyz, d_intensity (and d_poses with d_packet_poses) are required");
    auto misaligned = [](const void* p, uintptr_t a) { return p && ((uintptr_t) p % a) != 0; };
    if (misaligned(d_packets, 4) || misaligned(d_xyz, 16) || misaligned(d_intensity, 4) || misaligned(d_poses, 16) ||
        misaligned(d_packet_poses, 16) || misaligned(d_measurement_id, 4))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_decode: misaligned buffer (packets 4 B, xyz / poses / packet poses 16 B, intensity 4 B)");
    OUSTER_HIP_CHECK(hipSetDevice(o->device));
    DecodeArgs a;
    a.packets = d_packets;
    a.packet_poses = d_packet_poses;
    a.skip = d_skip;
    a.xyz = d_xyz;
    a.intensity = d_intensity;
    a.poses = d_poses;
    a.measurement_id = d_measurement_id;
    a.luts = o->d_luts;
    a.counters = o->d_counters;
    a.L = o->layout;
    a.H = o->rows;
    a.C = o->columns_per_packet;
    a.n_packets = n_packets;
    a.col_bytes = column_bytes(o->layout, o->rows);
    a.packet_bytes = o->packet_bytes;
    a.vec16 = ((uintptr_t) d_packets % 16 == 0) && (o->packet_bytes % 16 == 0);
    const size_t lds = (size_t) (o->packet_bytes + 15) / 16 * 16;
    hipLaunchKernelGGL(k_ouster_decode, dim3(n_packets, o->num_streams), dim3(BLOCK), lds, o->stream, a);
    OUSTER_HIP_CHECK(hipGetLastError());
    return CC_OK;
}

int cc_ouster_counters(cc_ouster* o, int stream, uint64_t* invalid_columns, uint64_t* bad_measurement_id, uint64_t* skipped_packets)
{
    if (!o || stream < 0 || stream >= o->num_streams)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_counters: no such stream");
    OUSTER_HIP_CHECK(hipSetDevice(o->device));
    OUSTER_HIP_CHECK(hipStreamSynchronize(o->stream));
    unsigned long long v[NUM_COUNTERS];
    OUSTER_HIP_CHECK(hipMemcpy(v, o->d_counters + (size_t) stream * NUM_COUNTERS, sizeof(v), hipMemcpyDeviceToHost));
    if (invalid_columns)
        *invalid_columns = v[CNT_INVALID];
    if (bad_measurement_id)
        *bad_measurement_id = v[CNT_BAD_MID];
    if (skipped_packets)
        *skipped_packets = v[CNT_SKIPPED];
    return CC_OK;
}

int cc_ouster_check_engine(cc_ouster* o, struct cc_engine* e)
{
    if (!o || !e)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_check_engine: null handle");
    cc_stream_state st;
    int rc = cc_engine_stream_state(e, o->num_streams - 1, &st);
    if (rc == CC_ERR_INVALID_ARGUMENT || (rc == CC_OK && cc_engine_stream_state(e, o->num_streams, &st) == CC_OK))
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_check_engine: the engine does not have " + std::to_string(o->num_streams) + " streams");
    if (rc != CC_OK)
        return fail(rc, std::string("cc_ouster_check_engine: ") + cc_engine_last_error(e));
    if (st.num_rows != o->rows)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_check_engine: the decoder has " + std::to_string(o->rows) + " rows, the engine " +
                                                 std::to_string(st.num_rows));
    return CC_OK;
}

int cc_ouster_make_lut(int columns_per_frame, int rows, double lidar_origin_to_beam_origin_mm, const double lidar_to_sensor_transform[16],
                       const double* azimuth_deg, const double* altitude_deg, float* direction, float* offset)
{
    if (columns_per_frame < 1 || rows < 1 || !lidar_to_sensor_transform || !azimuth_deg || !altitude_deg)
        return fail(CC_ERR_INVALID_ARGUMENT, "cc_ouster_make_lut: bad argument");
    const double* T = lidar_to_sensor_transform;
    const double range_unit = 0.001;
    const double azimuth_radians = M_PI * 2.0 / columns_per_frame;
    for (int v = 0; v < columns_per_frame; v++)
        for (int u = 0; u < rows; u++)
        {
            const double enc = 2.0 * M_PI - (v * azimuth_radians);
            const double az = -azimuth_deg[u] * M_PI / 180.0;
            const double alt = altitude_deg[u] * M_PI / 180.0;
            const double d[3] = {std::cos(enc + az) * std::cos(alt), std::sin(enc + az) * std::cos(alt), std::sin(alt)};
            const double f[3] = {(std::cos(enc) - d[0]) * lidar_origin_to_beam_origin_mm, (std::sin(enc) - d[1]) * lidar_origin_to_beam_origin_mm,
                                 (-d[2]) * lidar_origin_to_beam_origin_mm};
            const size_t i = ((size_t) v * rows + u) * 3;
            for (int j = 0; j < 3; j++)
            {
                const double rd = (d[0] * T[4 * j + 0] + d[1] * T[4 * j + 1]) + d[2] * T[4 * j + 2];
                const double ro = ((f[0] * T[4 * j + 0] + f[1] * T[4 * j + 1]) + f[2] * T[4 * j + 2]) + T[4 * j + 3];
                if (direction)
                    direction[i + j] = (float) (rd * range_unit);
                if (offset)
                    offset[i + j] = (float) (ro * range_unit);
            }
        }
    return CC_OK;
}

} // extern "C"
