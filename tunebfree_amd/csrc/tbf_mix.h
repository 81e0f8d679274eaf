/*
 * tbf_mix.h -- the arithmetic, member list and launch record of k_mix (csrc/tbf_mix.hip), shared
 * with its host side (csrc/tbf_mix.cpp) and with the host restatement tbf_debug_mix_ref, which runs
 * the same function.
 *
 * Definition (include/tbf.h): for bus b and frame j, over the rows r in ascending r with
 * bus[r] == b and j < count[r], from accL = accR = +0.0f,
 *     accL = fmaf (ll_r, L_r[j], accL);  accL = fmaf (lr_r, R_r[j], accL);
 *     accR = fmaf (rl_r, L_r[j], accR);  accR = fmaf (rr_r, R_r[j], accR);
 * one float32 fmaf per line, denormals kept, NaN and Inf literal, no term skipped for a zero
 * coefficient.  mix_term is those four lines.
 *
 * The host turns the caller's rows into a bus-sorted member list: busOff[b] .. busOff[b + 1] are
 * bus b's entries of `members`, their rows ascending, each with its coefficients and its count.
 */
#ifndef TBF_MIX_H
#define TBF_MIX_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/tbf.h"

#define TBF_MIX_LANES 64u        /* k_mix's workgroup: one wave */
#define TBF_MIX_GROUP 4u         /* the most frames a lane carries (one dwordx4 per plane and member) */
#define TBF_MIX_LOADS 32u        /* dwords of members' samples a lane keeps in flight */
#define TBF_MIX_CHUNK 64u        /* members staged in the wave's registers at a time: one per lane */
#define TBF_MIX_MAX_BUSES 65535u /* buses of one launch (the grid's y) */
#define TBF_MIX_FILL 2048u       /* waves a launch wants before a lane carries more than one frame */

#define TBF_MIX_HD __host__ __device__ __forceinline__

/* one member row's term of one frame */
TBF_MIX_HD void mix_term (float ll, float lr, float rl, float rr, float xl, float xr, float& accL, float& accR)
{
	accL = fmaf (ll, xl, accL);
	accL = fmaf (lr, xr, accL);
	accR = fmaf (rl, xl, accR);
	accR = fmaf (rr, xr, accR);
}

/* Frames per lane of a call: the widest group that still gives TBF_MIX_FILL waves, so that a long
 * call moves 16 B per load and a short call on few buses spreads over as many waves as it has
 * frames for.  The choice moves no bit: a frame's chain is the same in every lane. */
static inline uint32_t mix_frames_per_lane (uint64_t frames, uint64_t buses)
{
	for (uint32_t g = TBF_MIX_GROUP; g > 1u; g >>= 1) {
		const uint64_t tile = (uint64_t)TBF_MIX_LANES * g;
		if ((frames + tile - 1) / tile * buses >= TBF_MIX_FILL)
			return g;
	}
	return 1u;
}

/* a bus's member: 24 B */
typedef struct tbf_mix_member {
	uint32_t row;   /* its row of the input planes */
	uint32_t count; /* its valid frames; the kernel takes min (count, frames) */
	float    ll, lr, rl, rr;
} tbf_mix_member;

typedef struct tbf_mix_launch {
	const float*          in[2];    /* the L / R rows */
	uint64_t              inStride; /* floats between rows */
	float*                out[2];   /* bus b's frames from out[c] + b * outStride */
	uint64_t              outStride;
	const uint32_t*       busOff;   /* nBusesAll + 1 offsets into members */
	const tbf_mix_member* members;
	uint32_t              frames;   /* every output row's length */
	uint32_t              nBuses, busBase; /* buses of this launch (<= TBF_MIX_MAX_BUSES), the first one's number */
	uint32_t              group;    /* frames per lane: 4, 2 or 1 */
} tbf_mix_launch;

#endif
