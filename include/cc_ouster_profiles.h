/* cc_ouster_profiles.h — the UDP lidar profiles of the Ouster packet decoder (cc_ouster.h).
 *
 * The reference builds its packet_format from the udp_profile_lidar of the sensor's metadata (OusterInput, ros/ouster_input.hpp:57-92), so it
 * runs on whatever profile the sensor declares as long as that profile has the two fields it reads, RANGE and SIGNAL (:139-140).
 * cc_ouster_create makes a LEGACY decoder; cc_ouster_create_profile makes one for any profile below. One profile per handle (all streams of
 * a handle share rows and the [S][P][packet_bytes] layout), and such a handle works with every cc_ouster_* function of cc_ouster.h.
 *
 * Layouts (all fields little-endian; H = pixels_per_column, C = columns_per_packet). Restated from the Ouster SDK's packet_format and field
 * tables, which are not a dependency, and there are no recordings to check against: every profile is UNPINNED.
 *
 *                                      LEGACY                    RNG19_RFL8_SIG16_NIR16     RNG19_RFL8_SIG16_NIR16_DUAL
 *     packet header / footer bytes     0 / 0                     32 / 32                    32 / 32      (contents never looked at)
 *     column header bytes              16                        12                         12
 *     u64 timestamp / u16 m_id         @0 / @8                   @0 / @8                    @0 / @8
 *     status                           u32 after the last pixel  u16 @10 of the column      u16 @10 of the column
 *     column valid iff                 status & 1                status & 1                 status & 1
 *     pixel bytes                      12                        12                         16
 *     RANGE (mm)                       u32 @0 & 0x000FFFFF       u32 @0 & 0x0007FFFF        u32 @0 & 0x0007FFFF
 *     SIGNAL                           u16 @6                    u16 @6                     u16 @8
 *     never read                       refl u16 @4, nir u16 @8   flags in byte 2, refl u8   flags in byte 2, refl u8 @3, RANGE2 u32 @4,
 *                                                                @4, nir u16 @8             refl2 u8 @7, SIGNAL2 u16 @10, nir u16 @12
 *     column bytes                     16 + 12 H + 4             12 + 12 H                  12 + 16 H
 *     packet bytes                     C * column                32 + C * column + 32       32 + C * column + 32
 *     (H, C) = (32, 16) / (64, 16) / (128, 16):
 *                                      6464 / 12608 / 24896      6400 / 12544 / 24832       8448 / 16640 / 33024
 *
 * What a column produces is that of cc_ouster.h for every profile: the reference reads only RANGE and SIGNAL, so the second return of the
 * dual profile is ignored. RNG15_RFL8_NIR8 and FUSA_RNG15_RFL8_NIR8_DUAL have no SIGNAL field: the reference's ls.field(SIGNAL) cannot run
 * on them, and no intensity source is invented here; cc_ouster_profile_from_name knows the names and says so (-2).
 */
#ifndef CC_OUSTER_PROFILES_H
#define CC_OUSTER_PROFILES_H

#include "cc_ouster.h"

#ifdef __cplusplus
extern "C" {
#endif

enum
{
    CC_OUSTER_PROFILE_LEGACY = 0,
    CC_OUSTER_PROFILE_RNG19_RFL8_SIG16_NIR16 = 1,
    CC_OUSTER_PROFILE_RNG19_RFL8_SIG16_NIR16_DUAL = 2
};

/* cc_ouster_create with a profile; cc_ouster_create(...) is this with CC_OUSTER_PROFILE_LEGACY, except that this function also refuses
 * (CC_ERR_INVALID_ARGUMENT, the text names the packet size) a shape whose packet does not fit the 64 KB of LDS a workgroup stages it in,
 * e.g. C = 64, H = 128. Argument checks come before the device check: without a GPU a bad profile is CC_ERR_INVALID_ARGUMENT, a good one
 * CC_ERR_NO_DEVICE. */
int cc_ouster_create_profile(cc_ouster** out, int device, int num_streams, int rows, int columns_per_packet, int max_packets, int profile,
                             void* hip_stream);

/* Bytes of one packet of `profile`; 0 for an unknown profile, H < 1 or C < 1. (host only) */
int64_t cc_ouster_profile_packet_bytes(int profile, int rows, int columns_per_packet);

/* The enum of a metadata udp_profile_lidar string ("LEGACY", "RNG19_RFL8_SIG16_NIR16", "RNG19_RFL8_SIG16_NIR16_DUAL"); -1 for an unknown
 * name (or NULL); -2 for a known profile that has no SIGNAL field ("RNG15_RFL8_NIR8", "FUSA_RNG15_RFL8_NIR8_DUAL"). (host only) */
int cc_ouster_profile_from_name(const char* udp_profile_lidar);

/* The profile `o` was created with (0 for a handle of cc_ouster_create); -1 for NULL. */
int cc_ouster_profile_of(cc_ouster* o);

#ifdef __cplusplus
}
#endif
#endif
