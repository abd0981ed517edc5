/* cc_ouster.h — C-ABI of the Ouster lidar packet decoder that sits immediately upstream of insertion.
 *
 * The reference's live Ouster front end (OusterInput::onRawDataArrived, ros/ouster_input.hpp:105-181) turns every column of a
 * lidar packet into one firing on a host thread. This library does the same per-column decode as a HIP kernel on gfx950 and
 * writes the firings straight into the arrays cc_engine_add_firings_device (cc_hip.h) consumes, so packets go to HBM once and
 * never come back to the host. There is no CPU variant of the device path: cc_ouster_create fails with CC_ERR_NO_DEVICE without a GPU.
 *
 * cc_ouster_create makes a decoder of the LEGACY UDP profile, laid out below. The RNG19_RFL8_SIG16_NIR16 single- and dual-return profiles
 * (cc_ouster_create_profile and the other profile functions) are declared in cc_ouster_profiles.h; a handle made there works with every
 * function of this header, and what a column produces is the same for every profile.
 *
 * Packet layout, LEGACY UDP profile (all fields little-endian, no packet header or footer; H = pixels_per_column,
 * C = columns_per_packet). Restated from the Ouster SDK's packet_format, which is not a dependency: UNPINNED.
 *
 *     offset in column          field
 *     0                         u64 timestamp (ns)
 *     8                         u16 measurement_id  (m_id: the LUT column, 0 .. W-1)
 *     10                        u16 frame_id
 *     12                        u32 encoder_count
 *     16 + 12*row + 0           u32 range, low 20 bits (0x000FFFFF), millimetres
 *     16 + 12*row + 4           u16 reflectivity
 *     16 + 12*row + 6           u16 signal (the reference's intensity source)
 *     16 + 12*row + 8           u16 near-IR
 *     16 + 12*H                 u32 status (bit 0 set = valid column, ouster_input.hpp:120-125)
 *
 * column bytes = 16 + 12*H + 4, packet bytes = C * column bytes (6464 B for 32 x 16, 12608 B for 64 x 16).
 *
 * What one valid column (status & 1, m_id < W) of packet p of stream s produces (ouster_input.hpp:113-166): firing n = p*C + k with
 *     r = range & 0x000FFFFF;  r > 0: xyz[row] = (float) r * direction[m_id][row] + offset[m_id][row]  (f32, no FMA: SDK cartesianT)
 *                                      intensity[row] = (uint8_t) (fminf(1.f, (float) signal / 1000.f) * 255)
 *                              r == 0: xyz[row] = NaN, intensity[row] = 0
 * Row = beam index. The reference passes the DIRECTION block as the offset of cartesianT (:135-136), so its points are r*d + d: pass
 * the direction array as the offset LUT to reproduce it (cc_ouster_make_lut writes both, the caller chooses).
 *
 * An invalid column (status bit 0 clear), a column whose m_id >= W (the reference reads its LUT out of bounds there) and every column
 * of a packet marked in d_skip is written as an ALL-NaN firing (intensity 0, measurement id -1). The reference drops such columns; an
 * all-NaN firing changes nothing observable in the engine (no cell is filled, the rearmost / foremost columns do not move, nothing is
 * published), so labels, ids, events and published columns equal those of the dropped stream. Only firings_consumed and the
 * source_firing of a column view count the placeholders. d_skip is how a front end reproduces the reference's drop of
 * the packet after a reset (interrupt_message, :169-178) or pads a stream whose packet did not arrive in this slot.
 *
 * All device arrays are [num_streams][...] with the stream stride implied by n_packets of the call, exactly the layout of
 * cc_engine_add_firings_device for n = n_packets * C firings per stream. Functions return CC_OK (0) or a CC_ERR_* code of cc_hip.h;
 * cc_ouster_last_error() has the text.
 */
#ifndef CC_OUSTER_H
#define CC_OUSTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cc_ouster cc_ouster;

/* rows: pixels_per_column H (a multiple of 4, at most 128: Ouster sensors have 16 / 32 / 64 / 128 beams); it must equal the rows of the
 * engine the firings go to. columns_per_packet: C (16 on every Ouster sensor). max_packets: packets per stream one decode call may carry.
 * hip_stream: the hipStream_t the decode is enqueued on (pass cc_engine_hip_stream(e) and set the engine option "input_on_engine_stream"
 * to chain with an engine; destroy the decoder before that engine); NULL = own stream. */
int cc_ouster_create(cc_ouster** out, int device, int num_streams, int rows, int columns_per_packet, int max_packets, void* hip_stream);
void cc_ouster_destroy(cc_ouster* o);
const char* cc_ouster_last_error(void);
void* cc_ouster_hip_stream(cc_ouster* o);

/* The look-up table of `stream` (-1 = all streams): host arrays [W][H][3] of floats, indexed [measurement_id][row] (the order the
 * reference reorders the SDK's row-major table to, ouster_input.hpp:75-88). Streams given identical arrays share one device copy. */
int cc_ouster_set_lut(cc_ouster* o, int stream, int columns_per_frame, const float* direction, const float* offset);

/* Decode n_packets packets of every stream (asynchronous, on the handle's HIP stream). DEVICE pointers:
 *   d_packets         [S][n_packets][packet_bytes]  raw packets of the handle's profile (4-byte aligned; 16-byte alignment and a packet size
 *                                                   that is a multiple of 16 let the kernel use 16-B loads)
 *   d_packet_poses    [S][n_packets][12] doubles    odom_from_sensor of each packet, replicated to its C firings (:111: every firing of a
 *                                                   packet carries the packet's receive stamp); NULL = d_poses is left as the caller wrote it
 *   d_skip            [S][n_packets] uint8          nonzero: every column of the packet becomes an all-NaN firing; NULL = none
 *   d_xyz             [S][n_packets*C][H][3] float  (16-byte aligned)
 *   d_intensity       [S][n_packets*C][H] uint8     (4-byte aligned)
 *   d_poses           [S][n_packets*C][12] double   (16-byte aligned; may be NULL only with d_packet_poses NULL)
 *   d_measurement_id  [S][n_packets*C] int32        m_id of each firing, -1 for a placeholder; NULL = not wanted
 * Every stream needs a LUT (CC_ERR_INVALID_ARGUMENT otherwise). */
int cc_ouster_decode(cc_ouster* o, int n_packets, const uint8_t* d_packets, const double* d_packet_poses, const uint8_t* d_skip,
                     float* d_xyz, uint8_t* d_intensity, double* d_poses, int32_t* d_measurement_id);

/* Columns written as placeholders since create, per stream (synchronises): status bit 0 clear, m_id >= W (with a valid status), and
 * packets marked in d_skip (counted once per packet). Any pointer may be NULL. */
int cc_ouster_counters(cc_ouster* o, int stream, uint64_t* invalid_columns, uint64_t* bad_measurement_id, uint64_t* skipped_packets);
int cc_ouster_sync(cc_ouster* o);

/* Check that the firings of this decoder fit engine `e` (include cc_hip.h first): same number of streams, and H equal to the engine's
 * rows. CC_ERR_INVALID_ARGUMENT with a cc_ouster_last_error text otherwise. Synchronises the engine; call it once when pairing the two. */
struct cc_engine;
int cc_ouster_check_engine(cc_ouster* o, struct cc_engine* e);

/* ---- host-only helpers (plain C, no device) ------------------------------------------------------------------------------- */

/* C * (16 + 12 H + 4): bytes of one LEGACY packet; 0 for H < 1 or C < 1. */
int64_t cc_ouster_packet_bytes(int rows, int columns_per_packet);

/* The SDK's make_xyz_lut(info) (called by the reference at ouster_input.hpp:70), in double, cast to float (:71-72) and written in the
 * [W][H][3] order cc_ouster_set_lut takes. For column v, beam u:
 *     enc = 2 pi - v * (2 pi / W), az = -azimuth_deg[u] * pi / 180, alt = altitude_deg[u] * pi / 180
 *     dir = (cos(enc + az) cos(alt), sin(enc + az) cos(alt), sin(alt))
 *     off = (cos(enc) - dir.x, sin(enc) - dir.y, -dir.z) * lidar_origin_to_beam_origin_mm
 *     dir = R dir, off = R off + t (R, t: the 3x3 block and translation (mm) of the row-major 4x4 lidar_to_sensor_transform)
 *     dir, off *= 0.001 (range unit: mm -> m)
 * UNPINNED (restated without the SDK). direction / offset: [W][H][3] floats each; either may be NULL. */
int cc_ouster_make_lut(int columns_per_frame, int rows, double lidar_origin_to_beam_origin_mm, const double lidar_to_sensor_transform[16],
                       const double* azimuth_deg, const double* altitude_deg, float* direction, float* offset);

#ifdef __cplusplus
}
#endif
#endif
