/*
 * tbf_comp.h -- the arithmetic, constants and launch record of k_comp (csrc/tbf_comp.hip), shared
 * with its host side (csrc/tbf_comp.cpp) and with the host restatement tbf_debug_comp_ref, which
 * runs the same functions.
 *
 * Definition (include/tbf.h, "Bus compressor"): per row with its curve pt[0 .. 768], attack a,
 * release r, make-up m and state g (1.0f at creation), per frame n, every operation one float32
 * operation,
 *     p[n] = limit_peak (kL[n], kR[n])             csrc/tbf_limit.h; k the key pair, or the input
 *     t[n] = the curve at p[n]                     comp_lookup
 *     d    = g[n-1] - t[n];   g[n] = fmaf (d > 0 ? a : r, d, t[n])          comp_step
 *     y[n] = (g[n] * m) * x[n]  for each channel   comp_out
 */
#ifndef TBF_COMP_H
#define TBF_COMP_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/tbf.h"
#include "tbf_limit.h"

#define TBF_COMP_LANES 64u /* k_comp's workgroup: one wave */
#define TBF_COMP_TILE 128u /* frames of a row staged in LDS at a time */
#define TBF_COMP_GROUP 4u  /* frames between two LDS reads of a walking lane: one ds_read_b128 */
/* floats between the rows of an LDS plane: 4 more than the tile, so that the 16-byte reads of lanes
 * that stand at the same frame of consecutive rows fall on different banks (row l at 4 l mod 64), as
 * k_eq's and k_loud's */
#define TBF_COMP_PITCH (TBF_COMP_TILE + 4u)
/* floats between the curves in LDS: the points, rounded up to 16 B */
#define TBF_COMP_CURVE_PITCH ((TBF_COMP_POINTS + 3u) & ~3u)
/* the rows of a wave.  R is k_comp's template parameter; 4 is the one value built: 16 was built and
 * measured, and lost at every row count from 2 to 131072 */
#define TBF_COMP_ROWS 4u

#define TBF_COMP_HD __host__ __device__ __forceinline__

/* the rows a wave owns in an n_rows compressor */
TBF_COMP_HD constexpr uint32_t comp_rows (uint32_t) { return TBF_COMP_ROWS; }
/* LDS of a wave of R rows with n_curves curves, in floats: three planes (target / gain, L, R) of R
 * rows each, then the curves */
TBF_COMP_HD constexpr uint32_t comp_lds_plane (uint32_t R) { return R * TBF_COMP_PITCH; }
TBF_COMP_HD constexpr uint32_t comp_lds_floats (uint32_t R, uint32_t n_curves) { return 3u * comp_lds_plane (R) + n_curves * TBF_COMP_CURVE_PITCH; }

TBF_COMP_HD uint32_t comp_bits (float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __float_as_uint (x);
#else
	uint32_t u;
	memcpy (&u, &x, 4);
	return u;
#endif
}

/* the curve pt at the level p (>= 0, never NaN): 32 segments an octave from 2^-16 to 2^8, linear in
 * the mantissa's low 18 bits inside a segment; below the grid the first point, at and above its end
 * the last.  The index is clamped before the reads, so no level reads outside pt[0 .. 768]. */
TBF_COMP_HD float comp_lookup (const float* pt, float p)
{
	const uint32_t u  = comp_bits (p);
	int            i  = (int)(u >> 18) - (int)(111u << 5);
	i                 = i < 0 ? 0 : i > (int)TBF_COMP_POINTS - 2 ? (int)TBF_COMP_POINTS - 2 : i;
	const float    fr = (float)(u & 0x3FFFFu) * 0x1p-18f;
	const float    lo = pt[i], hi = pt[i + 1];
	const float    t  = fmaf (fr, hi - lo, lo);
	return p < 0x1p-16f ? pt[0] : p >= 0x1p8f ? pt[TBF_COMP_POINTS - 1u] : t;
}

/* one frame of the recurrence: the gain behind the target t, from the gain g before it */
TBF_COMP_HD float comp_step (float g, float t, float a, float r)
{
	const float d = g - t;
	return fmaf (d > 0.0f ? a : r, d, t);
}

/* one output sample: two multiplies, in this order */
TBF_COMP_HD float comp_out (float g, float m, float x) { return (g * m) * x; }

typedef struct tbf_comp_launch {
	const float*         in[2];  /* the L / R rows */
	const float*         key[2]; /* the key pair's rows, or both NULL: the input is the key */
	float*               out[2];
	uint64_t             inStride, keyStride, outStride; /* floats between rows */
	const uint32_t*      counts; /* every row's frames of this call, or NULL: `frames` each */
	const tbf_comp_row*  rows;   /* [row]: curve, attack, release, makeup */
	const float*         curves; /* [nCurves][TBF_COMP_POINTS] */
	float*               state;  /* [row]: g */
	tbf_comp_meter*      meters; /* [row], or NULL */
	uint32_t             frames;
	uint32_t             nCurves; /* 1..8 */
	uint32_t             nRows;
} tbf_comp_launch;

#endif
