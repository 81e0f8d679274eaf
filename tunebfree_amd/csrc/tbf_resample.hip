/*
 * tbf_resample.hip -- k_resample, the streaming polyphase rate converter behind L / R
 * (tbf_render_resampled* / tbf_process_resampled*, csrc/tbf_resample.cpp).
 *
 * The arithmetic is include/tbf.h's definition, through the functions of csrc/tbf_resample.h
 * that the host restatement runs too: per output one float32 fmaf per tap, t ascending, so a
 * row's outputs are the same bits however the render is cut.
 *
 * One workgroup of TBF_RS_LANES lanes owns one (instance, channel) row for the launch.  It walks
 * the row's outputs [C (P), C (P + nIn)) in tiles of TO; a lane carries up to TBF_RS_PER_LANE
 * outputs of a tile side by side (lane, lane + 256, ...: independent fmaf chains that overlap
 * each other's latency).  A tile's inputs, the T - 1 history samples in front of the call
 * included, are staged in LDS; when a tile's window would not fit TBF_RS_WINDOW floats (a long
 * filter: a steep downward ratio) the taps are walked in segments of TS, each with its own window,
 * the accumulators staying in the lanes' registers, and TO shrinks (csrc/tbf_resample.cpp picks
 * both).  The row's base C (P) * M is 64-bit, the offsets inside a tile 32-bit.
 * For L = 1 (UNI) there is one phase: the coefficient is wave-uniform and neighbouring lanes read
 * LDS at stride M.  Otherwise each lane walks its own phase row of the table.  The table is
 * phase-major and shared by every row; read from memory a wave's load touches 64 cache lines, which
 * measured 58 ms a step at 48000 -> 22050, so when it fits (TLDS: L * (T + 1) floats within
 * TBF_RS_TAB_LDS) each workgroup copies it into LDS once, rows at an odd stride.
 * At the end the row's last T - 1 inputs become its history; a call shorter than T - 1 shifts the
 * old history up instead of dropping it.  Reads of the old history and its overwrite are
 * separated by barriers: nothing else touches a row during a launch.
 * Rows are read inside [0, nIn) and written inside [0, C (P + nIn) - C (P)) only, one float at a
 * time.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbf_resample.h"

#define RS_R TBF_RS_PER_LANE

template <bool UNI, bool TLDS>
__global__ __launch_bounds__ (TBF_RS_LANES) void k_resample (tbf_rs_launch P)
{
	extern __shared__ __attribute__ ((aligned (16))) float smem[]; /* the window, then (TLDS) the table */
	float* const   win  = smem;
	const uint32_t lane = threadIdx.x, inst = blockIdx.x >> 1, ch = blockIdx.x & 1;
	const uint32_t L = UNI ? 1u : P.L, M = P.M, T = P.T, H = T - 1, nIn = P.nIn, TO = P.TO, TS = P.TS;
	const uint64_t pos  = P.pos ? P.pos[2 * (uint64_t)inst] : P.posU;      /* P at this launch's first input */
	const uint64_t pos0 = P.pos ? P.pos[2 * (uint64_t)inst + 1] : P.pos0U; /* P at the call's first input */
	const float* __restrict__ in = P.in[ch] + (uint64_t)inst * P.inStride;
	float* const hist = P.hist + ((uint64_t)inst * 2 + ch) * P.histFloats;
	const uint64_t n0  = rs_count (pos, L, M);
	const uint32_t cnt = (uint32_t)(rs_count (pos + nIn, L, M) - n0);
	float* const out   = P.out[ch] + (uint64_t)inst * P.outStride + (n0 - rs_count (pos0, L, M));
	const uint32_t grow = TBF_RS_ROW (T);
	const float*   tab  = P.tab;
	uint32_t       row  = grow;
	if (TLDS) { /* the table into LDS, rows at the odd stride P.ldsRow */
		float* const lt = smem + P.winFloats;
		row             = P.ldsRow;
		for (uint32_t k = lane; k < L * T; k += TBF_RS_LANES) {
			const uint32_t p = k / T, t = k - p * T;
			lt[p * row + t]  = P.tab[(uint64_t)p * grow + t];
		}
		tab = lt;
		__syncthreads ();
	}

	for (uint32_t j0 = 0; j0 < cnt; j0 += TO) {
		const uint32_t tn = min (TO, cnt - j0);
		/* the tile's first output: its input index and phase, in 64 bits; the lanes' offsets from it in 32 */
		const uint64_t pa = (n0 + j0) * M, ia = pa / L;
		const uint32_t fa = (uint32_t)(pa - ia * L);
		const int64_t  ra = (int64_t)(ia - pos);                  /* ia relative to the launch's first input: 0 .. nIn - 1 */
		const uint32_t span = (fa + (tn - 1) * M) / L + 1;        /* newest inputs of the tile's outputs: ia .. ia + span - 1 */
		uint32_t       irel[RS_R], phi[RS_R];
		float          acc[RS_R];
#pragma unroll
		for (int r = 0; r < RS_R; r++) { /* output lane + 256 r of the tile; beyond the tile: output 0 again, not stored */
			const uint32_t o = lane + r * TBF_RS_LANES, q = fa + (o < tn ? o : 0) * M;
			irel[r] = q / L;
			phi[r]  = q - irel[r] * L;
			acc[r]  = 0.0f;
		}
		for (uint32_t t0 = 0; t0 < T; t0 += TS) {
			const uint32_t nt = min (TS, T - t0);
			/* win[k] = x[ia - t0 - (TS - 1) + k], k < span + TS - 1: from the call's rows, the history, or
			 * (below the history: only beyond the last tap) zero */
			const int64_t  r0 = ra - (int64_t)t0 - (int64_t)(TS - 1);
			const uint32_t nw = span + TS - 1;
			for (uint32_t k = lane; k < nw; k += TBF_RS_LANES) {
				const int64_t r = r0 + (int64_t)k;
				float         v = 0.0f;
				if (r >= 0)
					v = in[r];
				else if (r >= -(int64_t)H)
					v = hist[(int64_t)H + r];
				win[k] = v;
			}
			__syncthreads ();
			const float* g[RS_R];
			const float* x[RS_R];
#pragma unroll
			for (int r = 0; r < RS_R; r++) {
				g[r] = tab + (uint64_t)phi[r] * row + t0;
				x[r] = win + irel[r] + TS - 1;
			}
			rs_taps_n<RS_R> (acc, g, x, nt);
			__syncthreads ();
		}
#pragma unroll
		for (int r = 0; r < RS_R; r++) {
			const uint32_t o = lane + r * TBF_RS_LANES;
			if (o < tn)
				out[j0 + o] = acc[r];
		}
	}
	/* the history for the next call: the last H of (old history, this launch's inputs) */
	__syncthreads ();
	for (uint32_t k0 = 0; k0 < H; k0 += TBF_RS_LANES) {
		const uint32_t k = k0 + lane;
		float          v = 0.0f;
		if (k < H) {
			const uint64_t s = (uint64_t)k + nIn; /* index into (old history, inputs) */
			v = s < H ? hist[s] : in[s - H];
		}
		__syncthreads (); /* this round's reads of the old history before its writes; later rounds read above them */
		if (k < H)
			hist[k] = v;
	}
}

template <bool UNI, bool TLDS>
static int rs_launch (const tbf_rs_launch& P, uint32_t ldsBytes, hipStream_t stream)
{
	/* only a launch that needs more dynamic LDS than every launch may have (48 KB) asks for it */
	if (ldsBytes > 48u * 1024u &&
	    hipFuncSetAttribute (reinterpret_cast<const void*> (&k_resample<UNI, TLDS>), hipFuncAttributeMaxDynamicSharedMemorySize,
	                         (int)ldsBytes) != hipSuccess)
		return -5;
	hipLaunchKernelGGL ((k_resample<UNI, TLDS>), dim3 (2 * P.n), dim3 (TBF_RS_LANES), ldsBytes, stream, P);
	return hipGetLastError () == hipSuccess ? 0 : -5;
}

extern "C" int tbf_launch_resample (const tbf_rs_launch* P, hipStream_t stream)
{
	if (P->n == 0 || P->nIn == 0)
		return 0;
	if (P->winFloats > TBF_RS_WINDOW || (P->ldsRow && (uint64_t)P->L * P->ldsRow > TBF_RS_TAB_LDS))
		return -5;
	if (P->L == 1)
		return rs_launch<true, false> (*P, P->winFloats * 4u, stream);
	if (P->ldsRow)
		return rs_launch<false, true> (*P, (P->winFloats + P->L * P->ldsRow) * 4u, stream);
	return rs_launch<false, false> (*P, P->winFloats * 4u, stream);
}
