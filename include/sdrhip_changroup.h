/* sdrhip_changroup.h — the channel group of libsdrhip.so: 1 to 8 handles of ONE node type of the channelizer family
 * (sdrhip_channelizer, sdrhip_chanaudio or sdrhip_chanpower; complex or real input, sdrhip_chanreal.h) served by ONE launch whose
 * second grid dimension is the member. An addition to sdrhip.h; the error codes and conventions are that header's.
 *
 * Why. One call of the family uses a fraction of the device (a 2^20-sample call at M = 1024 is 128 workgroups on 256 CUs), and
 * an application with several antennas, or with two grids on one antenna, enqueues such calls back to back. A group call puts
 * them into one launch.
 *
 * What a group is. It BORROWS its members, as sdrhip_rxbank borrows its components: they stay the caller's handles, must outlive
 * the group, and destroying the group leaves them as they are. A member's selection, modes, gains, thresholds, alpha and taps
 * keep working through its own setters, and so do its own process calls, in any order with the group's calls on the context's
 * stream. The members may differ in M, D, taps, selection and max_in; each has its own state. They share the context and the
 * input element type (the dtype, and real against complex), nothing else.
 *
 * What a group call computes. Member i is called exactly as its own process_dev would be with the i-th entries of the argument
 * arrays: the same rules (its own out_count, the stride rule with 0 = the call's count, its max_in), and afterwards its outputs
 * and its state are BIT FOR BIT what its own call would have left — the launch runs the member's kernel body on the member's
 * arguments, an output time is computed by the same operations in the same order, and the power monitor's workgroups walk the
 * tiles with the stride the member's own launch has (W = min(tiles, grid), whatever the group launch's grid is), so its sums,
 * levels and flags are the member's own as well.
 *
 * A member with n[i] = 0 is left out of the launch, its state untouched (its own call does nothing either); if every n is 0,
 * nothing is launched. EVERY rule of EVERY member is checked before anything is enqueued: a refused call changes no member — no
 * count moves, no byte is written. State moves on only behind an accepted launch.
 *
 * The launch (group_<family>[_real]_<type>_kernel): grid.x is the largest member's workgroup count in this call, grid.y the
 * members in the launch, 256 lanes, and the dynamic LDS is the largest member's (the group raises the kernel's limit at create
 * where a member needs more than 64 KiB). The member table travels by value in the kernel arguments and is indexed by
 * blockIdx.y. A workgroup whose x is beyond its member's tiles computes no tile and still rolls its share of that member's tail.
 * Nothing is synchronised.
 */
#ifndef SDRHIP_CHANGROUP_H
#define SDRHIP_CHANGROUP_H

#include "sdrhip.h"
#include "sdrhip_channelizer.h"
#include "sdrhip_chanaudio.h"
#include "sdrhip_chanpower.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the members of a group at most: four to eight calls of the family fill the device, and beyond that two group calls in a row
 * lose nothing */
#define SDRHIP_CHANGROUP_MAX 8

typedef struct sdrhip_changroup sdrhip_changroup;

/* members: count handles, copied (the handles are borrowed). Errors, checked in this order, the first two before anything is
 * dereferenced: NULL out / members SDRHIP_E_INVALID; count outside [1, SDRHIP_CHANGROUP_MAX] SDRHIP_E_SIZE; a NULL member
 * SDRHIP_E_INVALID (the message names its index); a member listed twice SDRHIP_E_INVALID; members on different contexts
 * SDRHIP_E_INVALID; members that differ in input element type (dtype, or real against complex) SDRHIP_E_INVALID. */
int sdrhip_changroup_channelizer_create(sdrhip_channelizer *const *members, int count, sdrhip_changroup **out);
int sdrhip_changroup_audio_create(sdrhip_chanaudio *const *members, int count, sdrhip_changroup **out);
int sdrhip_changroup_power_create(sdrhip_chanpower *const *members, int count, sdrhip_changroup **out);

/* The row call of a channelizer group (complex float rows) or an audio group (int16 rows); a power group: SDRHIP_E_INVALID.
 * Every array has `count` entries; n_out may be NULL, the other arrays not (SDRHIP_E_INVALID). Member i sees
 * (in_dev[i], n[i], out_dev[i], out_stride[i], &n_out[i]) under its own process_dev's rules. ONE launch on the context's stream.
 * Input extents may overlap or be the same pointer (one antenna on two grids). Every member's output extent must be disjoint from
 * every member's input extent and from every other member's output extent (SDRHIP_E_INVALID); outputs may lie back to back in one
 * buffer, which is how the rows of several antennas reach one downstream bank's process_dev in one block. */
int sdrhip_changroup_process_dev(sdrhip_changroup *g, const void *const *in_dev, const size_t *n, void *const *out_dev,
                                 const size_t *out_stride, size_t *n_out);

/* The call of a power group; any other group: SDRHIP_E_INVALID. in_dev and n have `count` entries; sum_dev may be NULL, and so
 * may any entry of it (only the state is wanted); n_out may be NULL. Member i sees (in_dev[i], n[i], sum_dev[i], &n_out[i]) under
 * sdrhip_chanpower_process_dev's rules; a sum row must be disjoint from every member's input and every other sum row
 * (SDRHIP_E_INVALID). TWO launches: the main kernel, and one finish launch (group_chanpower_finish_kernel, grid.y = the member)
 * over the members that need one — a member that alone would skip its finish launch (no outputs and no sums asked for) skips it
 * here too. calls, alpha, the output count and `first` are per member. */
int sdrhip_changroup_power_process_dev(sdrhip_changroup *g, const void *const *in_dev, const size_t *n, double *const *sum_dev,
                                       size_t *n_out);

/* any pointer may be NULL: the members; grid_x, the launch's first grid dimension where every member is called with its max_in
 * (a power group: the largest member's grid); lds_bytes, the launch's dynamic LDS: the largest member's */
int sdrhip_changroup_plan_info(sdrhip_changroup *g, int *members, int *grid_x, int *lds_bytes);
/* the kernels of a group call, comma-separated: "group_channelizer_cs16_kernel", "group_chanaudio_real_f32_kernel",
 * "group_chanpower_cf32_kernel,group_chanpower_finish_kernel", ... */
int sdrhip_changroup_kernel_names(sdrhip_changroup *g, char *buf, size_t len);
/* the members are left as they are */
int sdrhip_changroup_destroy(sdrhip_changroup *g);

#ifdef __cplusplus
}
#endif
#endif
