/*
 * tbf_tpeak.hip -- k_tpeak, the oversampled peaks of the true-peak meter beside any two float32
 * planes (tbf_true_peak_device, csrc/tbf_tpeak.cpp): per row and channel the largest magnitude of
 * the samples and of the F - 1 (F = 2) or 4 (F = 4) interpolated values per frame.
 *
 * The arithmetic is include/tbf.h's definition through tpeak_y and tpeak_mag of csrc/tbf_tpeak.h,
 * which the host restatement runs too.  Every interpolated value is a chain of 12 fmaf over the 12
 * newest frames and a maximum of bit patterns is exact in any order, so the kernel is parallel over
 * rows and over time: a workgroup of TBF_TPEAK_LANES = 256 lanes takes one tile of TBF_TPEAK_TILE =
 * 1024 consecutive frames of one row, blockIdx.x = row * tiles + tile.
 *   Staging.  Lane l loads frames l, l + 256, l + 512, l + 768 of the tile of both channels (four
 * waves on 256 consecutive dwords: coalesced, and dword loads because the pointers are only 4-byte
 * aligned) and lanes 1 .. 11 the 11 frames in front of the tile: from the planes when the tile is
 * not the row's first of this call, else from the live side of the row's history.  A frame at or
 * beyond the row's count is not read; its LDS word is +0.0f.
 *   LDS: tile[channel][TBF_TPEAK_CHAN] floats, a channel's word i holding frame t0 - 12 + i (word 0
 * is never used).  Lane l then owns frames 4 l .. 4 l + 3 of the tile and reads words 4 l ..
 * 4 l + 15 as four aligned 16-byte values (consecutive lanes 16 B apart; the compiler reads them as
 * eight ds_read2_b32), which are the 15 frames its four windows cover.  Per channel that is 4 frames x F phases x 12 v_fma_f32, every chain
 * in tap order, with the coefficients as literals.
 *   Peaks.  A frame at or beyond the count contributes 0, the identity of the unsigned maximum.  The
 * four maxima are reduced over the wave by shuffles, over the four waves through 16 words of LDS,
 * and lanes 0 .. 3 issue one vector atomicMax each on the row's four words (none for a 0).
 *   History.  The workgroup of the tile that holds the row's last frame writes the row's other side:
 * the last 11 of (live side || the frames taken), from the live side and from the planes.  Every
 * workgroup of the call reads the live side only and the host flips the side of the rows that took
 * frames, so a call's reads and writes of the history never meet, whatever order the workgroups run in.
 *
 * Bounds.  Rows: blockIdx.x / tiles < nRows by the grid.  Global reads: in[ch][row * inStride + f]
 * with f < count <= frames <= inStride (checked by the host): the tile's frames are tested against
 * count, the halo's frames t0 - 11 .. t0 - 1 are below t0 < count, the history writer's frames
 * count - 11 + i are tested >= 0 and are below count.  t0 + 1023 does not wrap: t0 is a multiple of
 * 1024 below 2^32.  History: hist[(row * 2 + side) * 22 + ch * 11 + i], side < 2, ch < 2, i < 11; the
 * old side's index 11 + s has -11 <= s < 0.  Peaks: peaks[row * 4 + lane], lane < 4.  LDS: ch * CHAN
 * + i with i < 12 (halo), 12 + k * 256 + lane < CHAN (tile), 4 lane + 15 <= 1035 < CHAN (window);
 * part[wave][k] with wave < 4, k < 4.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbf_tpeak.h"

#define TPEAK_WAVES (TBF_TPEAK_LANES / 64u)
#define TPEAK_LOADS (TBF_TPEAK_TILE / TBF_TPEAK_LANES) /* dwords a lane loads per channel */

template <uint32_t F> __global__ __launch_bounds__ (TBF_TPEAK_LANES) void k_tpeak (tbf_tpeak_launch P)
{
	__shared__ float4   lds4[2u * TBF_TPEAK_CHAN / 4u];
	__shared__ uint32_t part[TPEAK_WAVES][4];
	float* const        tile = reinterpret_cast<float*> (lds4);

	const uint32_t      lane = threadIdx.x;
	const uint32_t      row = blockIdx.x / P.tiles, t = blockIdx.x % P.tiles;
	const tbf_tpeak_row rw    = P.rows[row];
	const uint32_t      count = rw.count, t0 = t * TBF_TPEAK_TILE;
	if (t0 >= count) /* the whole workgroup: this row takes fewer tiles than the longest */
		return;
	const float* const hOld = P.hist + ((uint64_t)row * 2u + (rw.side & 1u)) * (2u * TBF_TPEAK_HIST);
	float* const       hNew = P.hist + ((uint64_t)row * 2u + ((rw.side & 1u) ^ 1u)) * (2u * TBF_TPEAK_HIST);

	/* the tile and its halo: all loads first, then the LDS stores */
	float v[2][TPEAK_LOADS], halo[2] = {0.0f, 0.0f};
#pragma unroll
	for (uint32_t ch = 0; ch < 2u; ch++) {
		const float* const src = P.in[ch] + (uint64_t)row * P.inStride;
#pragma unroll
		for (uint32_t k = 0; k < TPEAK_LOADS; k++) {
			const uint32_t f = t0 + k * TBF_TPEAK_LANES + lane;
			v[ch][k]         = f < count ? src[f] : 0.0f;
		}
		if (lane >= 1u && lane < TBF_TPEAK_HALO)
			halo[ch] = t0 ? src[t0 - TBF_TPEAK_HALO + lane] : hOld[ch * TBF_TPEAK_HIST + lane - 1u];
	}
#pragma unroll
	for (uint32_t ch = 0; ch < 2u; ch++) {
#pragma unroll
		for (uint32_t k = 0; k < TPEAK_LOADS; k++)
			tile[ch * TBF_TPEAK_CHAN + TBF_TPEAK_HALO + k * TBF_TPEAK_LANES + lane] = v[ch][k];
		if (lane < TBF_TPEAK_HALO)
			tile[ch * TBF_TPEAK_CHAN + lane] = halo[ch];
	}
	__syncthreads ();

	/* m: sample L, sample R, inter L, inter R */
	uint32_t       m[4] = {0u, 0u, 0u, 0u};
	const uint32_t f0   = t0 + TBF_TPEAK_PER_LANE * lane; /* the lane's first frame */
#pragma unroll
	for (uint32_t ch = 0; ch < 2u; ch++) {
		const float4* const q = reinterpret_cast<const float4*> (tile + ch * TBF_TPEAK_CHAN + TBF_TPEAK_PER_LANE * lane);
		const float4        a = q[0], b = q[1], c = q[2], d = q[3];
		const float         w[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w};
#pragma unroll
		for (uint32_t i = 0; i < TBF_TPEAK_PER_LANE; i++) {
			const bool take = f0 + i < count; /* f0 + i <= t0 + 1023: no wrap */
			m[ch]           = max (m[ch], take ? tpeak_mag (w[TBF_TPEAK_HALO + i]) : 0u);
#pragma unroll
			for (uint32_t p = 0; p < tpeak_phases (F); p++) {
				const float y = tpeak_y (tpeak_phase (F, p), &w[TBF_TPEAK_HALO + i]);
				m[2u + ch]    = max (m[2u + ch], take ? tpeak_mag (y) : 0u);
			}
		}
	}

	/* over the wave, over the workgroup, and into the row's words */
#pragma unroll
	for (uint32_t k = 0; k < 4u; k++)
#pragma unroll
		for (int d = 32; d; d >>= 1)
			m[k] = max (m[k], (uint32_t)__shfl_xor ((int)m[k], d));
	if ((lane & 63u) == 0u) {
#pragma unroll
		for (uint32_t k = 0; k < 4u; k++)
			part[lane / 64u][k] = m[k];
	}
	__syncthreads ();
	if (lane < 4u) {
		uint32_t mx = part[0][lane];
#pragma unroll
		for (uint32_t wv = 1; wv < TPEAK_WAVES; wv++)
			mx = max (mx, part[wv][lane]);
		if (mx)
			atomicMax (P.peaks + (uint64_t)row * 4u + lane, mx);
	}

	/* the row's new history, by the workgroup of its last frame */
	if (t == (count - 1u) / TBF_TPEAK_TILE && lane < 2u * TBF_TPEAK_HIST) {
		const uint32_t ch = lane / TBF_TPEAK_HIST, i = lane % TBF_TPEAK_HIST;
		const int64_t  s = (int64_t)count - (int64_t)TBF_TPEAK_HIST + (int64_t)i; /* the frame of this call, or < 0: one of before */
		hNew[lane]       = s < 0 ? hOld[ch * TBF_TPEAK_HIST + (uint32_t)((int64_t)TBF_TPEAK_HIST + s)]
		                         : P.in[ch][(uint64_t)row * P.inStride + (uint64_t)s];
	}
}

extern "C" int tbf_launch_tpeak (const tbf_tpeak_launch* P, hipStream_t stream)
{
	if (P->nRows == 0 || P->tiles == 0)
		return 0;
	if (!P->in[0] || !P->in[1] || !P->rows || !P->hist || !P->peaks)
		return -5;
	const uint64_t groups = (uint64_t)P->nRows * P->tiles;
	if (groups > 0x7fffffffull)
		return -5;
	const dim3 grid ((uint32_t)groups), block (TBF_TPEAK_LANES);
	switch (P->F) {
	case 1u: hipLaunchKernelGGL (k_tpeak<1u>, grid, block, 0, stream, *P); break;
	case 2u: hipLaunchKernelGGL (k_tpeak<2u>, grid, block, 0, stream, *P); break;
	case 4u: hipLaunchKernelGGL (k_tpeak<4u>, grid, block, 0, stream, *P); break;
	default: return -5;
	}
	return hipGetLastError () == hipSuccess ? 0 : -5;
}
