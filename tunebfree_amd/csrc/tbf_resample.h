/*
 * tbf_resample.h -- the arithmetic, layout and launch record of k_resample
 * (csrc/tbf_resample.hip), shared with its host side (csrc/tbf_resample.cpp) and with the host
 * restatement tbf_debug_resample_ref, which runs the same functions with libm's fmaf.
 *
 * Definition (include/tbf.h): L / M = Fo / Fi in lowest terms, T taps per phase, the prototype
 * g[k], k = 0 .. L T - 1.  Output n of a row: p = n M, i = p div L, phi = p mod L,
 *     y[n] = fmaf (g[phi + (T-1) L], x[i-(T-1)], ... fmaf (g[phi + L], x[i-1], fmaf (g[phi], x[i], 0)))
 * one float32 fmaf per tap, t ascending.  The table is stored phase-major: row phi holds
 * g[phi + t L], t = 0 .. T - 1, at tab + phi * TBF_RS_ROW (T) (rows padded to four floats, the
 * padding never read as a tap).
 * State per instance and channel: the last T - 1 inputs, oldest first, in TBF_RS_HIST (T) floats.
 */
#ifndef TBF_RESAMPLE_H
#define TBF_RESAMPLE_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define TBF_RS_ZC 32                  /* zero crossings a side */
#define TBF_RS_MAX_L 1024u            /* the cap: L, and L * T */
#define TBF_RS_MAX_TABLE (1u << 18)
#define TBF_RS_LANES 256u             /* k_resample's workgroup */
#define TBF_RS_PER_LANE 4             /* outputs a lane carries side by side */
#define TBF_RS_WINDOW 8192u           /* floats of LDS a tile's inputs may take */
#define TBF_RS_TAB_LDS 30720u         /* floats of LDS the phase table may take (120 KB); beyond: read from memory */

#define TBF_RS_PAD4(v) (((uint32_t)(v) + 3u) & ~3u)
#define TBF_RS_HIST(T) TBF_RS_PAD4 ((T) - 1u)
#define TBF_RS_ROW(T) TBF_RS_PAD4 (T)

#define TBF_RS_HD __host__ __device__ __forceinline__

/* C (P) = ceil (P L / M): the outputs that exist after P inputs */
TBF_RS_HD uint64_t rs_count (uint64_t P, uint32_t L, uint32_t M) { return (P * L + M - 1) / M; }

/* nt taps of R outputs side by side, continuing acc[r]: g[r] the output's phase row from its tap
 * t0 on, x[r] the input that tap t0 meets (x[r][0], then x[r][-1], ...).  Every output is its own
 * chain of fmafs in ascending t; R only lets independent chains overlap. */
template <int R>
TBF_RS_HD void rs_taps_n (float (&acc)[R], const float* const (&g)[R], const float* const (&x)[R], uint32_t nt)
{
#pragma unroll 4
	for (uint32_t t = 0; t < nt; t++)
#pragma unroll
		for (int r = 0; r < R; r++)
			acc[r] = fmaf (g[r][t], x[r][-(int32_t)t], acc[r]);
}

/* one output: what the host restatement runs */
TBF_RS_HD float rs_taps (float acc, const float* g, const float* x, uint32_t nt)
{
	float              a[1]  = {acc};
	const float* const gg[1] = {g};
	const float* const xx[1] = {x};
	rs_taps_n<1> (a, gg, xx, nt);
	return a[0];
}

typedef struct tbf_rs_launch {
	const float*    in[2];     /* the engine-rate L / R rows of the call (or piece) */
	uint64_t        inStride;
	float*          out[2];    /* the converted rows, from the call's first output of each instance */
	uint64_t        outStride;
	float*          hist;      /* instance i, channel c at hist + (2 i + c) * histFloats */
	const float*    tab;       /* [L][TBF_RS_ROW (T)] */
	const uint64_t* pos;       /* per instance (P at the piece's start, P at the call's start), or NULL: */
	uint64_t        posU, pos0U; /* ... the same two for every instance */
	uint32_t        n, nIn;    /* instances, input samples per row */
	uint32_t        L, M, T, histFloats;
	uint32_t        TO, TS;    /* outputs per tile (<= TBF_RS_LANES * TBF_RS_PER_LANE), taps per staged segment */
	uint32_t        winFloats; /* LDS floats of a tile's window: the tile's span + TS - 1 */
	uint32_t        ldsRow;    /* L > 1: the table's row stride in LDS (odd: the lanes' rows spread over the banks), 0: not in LDS */
} tbf_rs_launch;

#endif
