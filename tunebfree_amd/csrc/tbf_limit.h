/*
 * tbf_limit.h -- the arithmetic, constants and launch record of k_limit (csrc/tbf_limit.hip),
 * shared with its host side (csrc/tbf_limit.cpp) and with the host restatement
 * tbf_debug_limit_ref, which runs the same functions.
 *
 * Definition (include/tbf.h): with ceiling c, look-ahead A (a power of two), hold H, W = A + H,
 * D = A - 1, and all frames before a row's first +0.0f,
 *     p[n] = the larger of fabsf (xL[n]), fabsf (xR[n]), NaN skipped      limit_peak
 *     t[n] = p[n] > c ? c / p[n] : 1.0f                                  limit_target
 *     m[n] = min (t[n-W+1] .. t[n])
 *     g[n] = (m[n-A+1] + ... + m[n]) * (1.0f / A), the sum ascending from +0.0f, one add a term
 *     y[n] = clamp (g[n] * x[n-D], -c, c), NaN kept                       limit_out
 * g[n] reaches back A + W - 2 = Hn frames, which is the history a row keeps per channel.
 */
#ifndef TBF_LIMIT_H
#define TBF_LIMIT_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/tbf.h"
#include "tbf_tpeak.h"

#define TBF_LIMIT_LANES 256u       /* k_limit's workgroup */
#define TBF_LIMIT_GROUP 4u         /* consecutive frames a lane carries: one dwordx4 per plane */
#define TBF_LIMIT_SUB (TBF_LIMIT_LANES * TBF_LIMIT_GROUP) /* frames of one pass of the workgroup */
#define TBF_LIMIT_MAX_ROWS 65535u  /* rows of one launch (the grid's y) */

#define TBF_LIMIT_HD __host__ __device__ __forceinline__

/* the frames of history per row and channel */
TBF_LIMIT_HD uint32_t limit_history (uint32_t ahead, uint32_t hold) { return 2u * ahead + hold - 2u; }

/* Frames of a workgroup's tile: one pass of the workgroup while the halo (Hn frames in front of
 * the tile, staged again by every tile) is no longer than that, two beyond.  A function of the
 * configuration alone, and no choice moves a bit. */
TBF_LIMIT_HD uint32_t limit_tile (uint32_t ahead, uint32_t hold)
{
	return limit_history (ahead, hold) <= TBF_LIMIT_SUB ? TBF_LIMIT_SUB : 2u * TBF_LIMIT_SUB;
}

/* floats of one of the kernel's two LDS arrays: the tile and its halo, room for the window
 * minima's alignment shift, rounded to 16 B */
TBF_LIMIT_HD uint32_t limit_lds_floats (uint32_t ahead, uint32_t hold)
{
	return (limit_tile (ahead, hold) + limit_history (ahead, hold) + 8u + 3u) & ~3u;
}

TBF_LIMIT_HD float limit_peak (float xl, float xr)
{
	float p = 0.0f;
	if (fabsf (xl) > p)
		p = fabsf (xl);
	if (fabsf (xr) > p)
		p = fabsf (xr);
	return p;
}

TBF_LIMIT_HD float limit_target (float p, float c) { return p > c ? c / p : 1.0f; }

/* one output sample; clamped counts the samples the clamp replaced */
TBF_LIMIT_HD float limit_out (float g, float x, float c, uint32_t& clamped)
{
	float y = g * x;
	if (y > c) {
		y = c;
		clamped++;
	}
	if (y < -c) {
		y = -c;
		clamped++;
	}
	return y;
}

/* ---- the true-peak detector (tbf_limiter_create_tp, k_limit_tp of csrc/tbf_limit_tp.hip) ----
 * Definition (include/tbf.h): with oversampling F in {2, 4}, E = 6 and the meter's chains yc[n][q]
 * (tpeak_y of csrc/tbf_tpeak.h over xc[n-11 .. n]),
 *     p[n] = the largest of fabsf (xL[n-E]), fabsf (xR[n-E]) and fabsf (yc[n][q]) of both channels and
 *            every phase F uses, NaN skipped                                limit_tp_peak
 *     t, m, g as above;  y[n] = limit_out (g[n], x[n-D-E], c)
 * t[n] reaches x[n-11], so the history grows by 11 frames and the latency by E. */
#define TBF_LIMIT_TP_DELAY 6u                     /* E */
#define TBF_LIMIT_TP_REACH (TBF_TPEAK_TAPS - 1u)  /* the frames behind n that t[n] reads */
/* k_limit_tp stages the raw samples a pass of the workgroup at a time: per channel TBF_LIMIT_SUB
 * frames behind the 11 in front of them and one unused word, so that lane l's 16 floats are four
 * aligned 16-byte values, as in k_tpeak */
#define TBF_LIMIT_TP_HALO 12u
#define TBF_LIMIT_TP_RAW (TBF_LIMIT_SUB + TBF_LIMIT_TP_HALO)

TBF_LIMIT_HD uint32_t limit_tp_history (uint32_t ahead, uint32_t hold) { return limit_history (ahead, hold) + TBF_LIMIT_TP_REACH; }

/* the workgroup's LDS bytes: k_limit's two arrays and the raw samples of one pass, L and R */
TBF_LIMIT_HD uint32_t limit_tp_lds_bytes (uint32_t ahead, uint32_t hold)
{
	return (2u * limit_lds_floats (ahead, hold) + 2u * TBF_LIMIT_TP_RAW) * (uint32_t)sizeof (float);
}

/* p[n] from nl = &xL[n], nr = &xR[n], each with x[n - j] at [-j], j < 12.  The maximum of values
 * that are no NaN is exact in any order. */
TBF_LIMIT_HD float limit_tp_peak (uint32_t F, const float* nl, const float* nr)
{
	float p = limit_peak (nl[-(int)TBF_LIMIT_TP_DELAY], nr[-(int)TBF_LIMIT_TP_DELAY]);
#if defined(__HIP_DEVICE_COMPILE__) /* the kernel's F is a constant; the host restatement's is not */
#pragma unroll
#endif
	for (uint32_t q = 0; q < tpeak_phases (F); q++) {
		const float yl = tpeak_y (tpeak_phase (F, q), nl), yr = tpeak_y (tpeak_phase (F, q), nr);
		if (fabsf (yl) > p)
			p = fabsf (yl);
		if (fabsf (yr) > p)
			p = fabsf (yr);
	}
	return p;
}

/* a row of a call: 8 B */
typedef struct tbf_limit_row {
	uint32_t count; /* its frames of this call */
	uint32_t side;  /* which of its two history buffers holds its state: the call reads it and writes the other */
} tbf_limit_row;

typedef struct tbf_limit_launch {
	const float*         in[2];    /* the L / R rows */
	uint64_t             inStride; /* floats between rows */
	float*               out[2];
	uint64_t             outStride;
	float*               hist;     /* [row][side][channel][Hn], Hn_tp for k_limit_tp */
	const tbf_limit_row* rows;     /* every row of the limiter */
	tbf_limit_meter*     meters;   /* or NULL */
	float                ceiling;
	uint32_t             ahead, hold;
	uint32_t             maxCount; /* the largest count of the launch's rows */
	uint32_t             nRows, rowBase; /* rows of this launch (<= TBF_LIMIT_MAX_ROWS), the first one's number */
} tbf_limit_launch;

#endif
