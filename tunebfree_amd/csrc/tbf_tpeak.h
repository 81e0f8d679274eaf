/*
 * tbf_tpeak.h -- the table, the arithmetic, constants and launch record of k_tpeak
 * (csrc/tbf_tpeak.hip), shared with its host side (csrc/tbf_tpeak.cpp) and with the host
 * restatement tbf_debug_true_peak_ref, which runs the same functions.
 *
 * Definition (include/tbf.h, "True-peak meter"): the 4-phase, 12-tap interpolator of ITU-R BS.1770-4
 * Annex 2, h[p][j] = k[p][j] / 8192 with k[2], k[3] the reverses of k[1], k[0].  Per row, channel,
 * input frame n and phase p used,
 *     acc = +0.0f;  for j = 0 .. 11 ascending:  acc = fmaf (h[p][j], x[n - j], acc);  y[n][p] = acc
 * and the peaks are the unsigned maxima of the magnitudes' bit patterns (tpeak_mag) of every x[n]
 * and of every y[n][p].
 */
#ifndef TBF_TPEAK_H
#define TBF_TPEAK_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/tbf.h"

#define TBF_TPEAK_TAPS 12u
#define TBF_TPEAK_HIST (TBF_TPEAK_TAPS - 1u) /* frames of a channel a row keeps between calls */
#define TBF_TPEAK_LANES 256u                 /* k_tpeak's workgroup: four waves */
#define TBF_TPEAK_PER_LANE 4u                /* consecutive frames of a lane */
#define TBF_TPEAK_TILE (TBF_TPEAK_LANES * TBF_TPEAK_PER_LANE) /* frames of a row a workgroup takes */
/* floats of a channel in LDS in front of the tile's first frame: the 11 frames before it behind one
 * unused word, so that lane l's window (frames 4 l - 12 .. 4 l + 3 of the tile) is four aligned
 * 16-byte values */
#define TBF_TPEAK_HALO 12u
#define TBF_TPEAK_CHAN (TBF_TPEAK_TILE + TBF_TPEAK_HALO) /* floats of a channel in LDS */
#define TBF_TPEAK_LDS_BYTES (2u * TBF_TPEAK_CHAN * 4u + 4u * 4u * 4u) /* the tile and the waves' partial maxima */
/* floats of history a row holds: two sides (the live one and the one the next call writes), each
 * L's 11 frames and then R's, oldest first */
#define TBF_TPEAK_ROW_HIST (2u * 2u * TBF_TPEAK_HIST)

#define TBF_TPEAK_HD __host__ __device__ __forceinline__

/* h[p][j]: an integer of at most 13 bits over 2^13, exact in float32 */
TBF_TPEAK_HD float tpeak_h (uint32_t p, uint32_t j)
{
	constexpr int k0[TBF_TPEAK_TAPS] = {14, 90, -161, 272, -487, 1125, 7964, -838, 390, -218, 122, -68};
	constexpr int k1[TBF_TPEAK_TAPS] = {-239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155};
	const int     k = p == 0u ? k0[j] : p == 1u ? k1[j] : p == 2u ? k1[TBF_TPEAK_TAPS - 1u - j] : k0[TBF_TPEAK_TAPS - 1u - j];
	return (float)k * (1.0f / 8192.0f);
}

/* the q-th phase a meter of oversampling factor F uses, q < F - (F == 1) */
TBF_TPEAK_HD uint32_t tpeak_phase (uint32_t F, uint32_t q) { return F == 4u ? q : 2u * q; }
/* the phases a factor uses: none at F = 1, where only the samples are taken */
TBF_TPEAK_HD uint32_t tpeak_phases (uint32_t F) { return F == 1u ? 0u : F; }

/* y[n][p] from newest = &x[n], with x[n - j] at newest[-j]: the chain in tap order */
TBF_TPEAK_HD float tpeak_y (uint32_t p, const float* newest)
{
	float acc = 0.0f;
#pragma unroll
	for (uint32_t j = 0; j < TBF_TPEAK_TAPS; j++)
		acc = fmaf (tpeak_h (p, j), newest[-(int)j], acc);
	return acc;
}

/* the bit pattern of |v|: as unsigned integers these order the finite magnitudes as floats do, put
 * Inf above them and every NaN above Inf */
TBF_TPEAK_HD uint32_t tpeak_mag (float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __float_as_uint (v) & 0x7fffffffu;
#else
	uint32_t u;
	memcpy (&u, &v, sizeof (u));
	return u & 0x7fffffffu;
#endif
}

/* one row of a call: the frames it takes and which side of its history is live */
typedef struct tbf_tpeak_row {
	uint32_t count, side;
} tbf_tpeak_row;

typedef struct tbf_tpeak_launch {
	const float*         in[2];    /* the L / R rows */
	uint64_t             inStride; /* floats between rows */
	const tbf_tpeak_row* rows;     /* [nRows] */
	float*               hist;     /* [row][side][channel][11] */
	uint32_t*            peaks;    /* [row]{sample L, sample R, inter L, inter R} */
	uint32_t             nRows;
	uint32_t             tiles;    /* workgroups a row: ceil (largest count / TILE) */
	uint32_t             F;        /* 1, 2 or 4 */
} tbf_tpeak_launch;

#endif
