/*
 * tbf_comp.hip -- k_comp, the bus compressor behind any two float32 planes (tbf_comp_device,
 * csrc/tbf_comp.cpp): per row a gain that follows a target read from a curve, by a float32
 * recurrence with an attack and a release coefficient, times a make-up, on both channels.
 *
 * The arithmetic is include/tbf.h's definition through comp_lookup, comp_step and comp_out of
 * csrc/tbf_comp.h, which the host restatement runs too.  Of a frame's work only the recurrence
 * g[n] = fmaf (g[n-1] - t[n] > 0 ? a : r, g[n-1] - t[n], t[n]) depends on the frame before it; the
 * detector, the curve and the output multiply do not.  So the kernel splits the frame: everything
 * but the recurrence runs with the wave's 64 lanes on 64 consecutive frames of a row, and the
 * recurrence alone runs with one lane per row.  Nothing is re-associated: every operation is the
 * definition's, and the order in which independent frames are computed is not observable.
 *
 * A workgroup is one wave and owns R consecutive rows.  R is a template parameter and 4 the one
 * value built (TBF_COMP_ROWS): a wave's walk costs the same whether 1 or 64 of its lanes walk, so
 * few rows a wave put more of the machine to walking; R = 16 was built too and lost at every row
 * count measured, 2 to 131072.  Lane l < R holds row l's parameters and
 * its g in registers from one load at entry to one store at exit.  The curves of the compressor
 * are copied into LDS once, at entry.  The wave walks tiles of TBF_COMP_TILE = 128 frames:
 *   1. Stage.  The tile's L and R, and the key pair's when the call has one, were loaded into
 *      registers with coalesced loads (64 lanes on 64 consecutive frames of one row: 256 B an
 *      instruction) while the tile before was walked.  L and R go to two LDS planes, where they
 *      wait for phase 4, and the registers are free for the next tile's loads, which are issued
 *      before the walk.  A frame at or beyond its row's count is not read: the load goes to the
 *      curves' first point instead (comp_fetch), so all loads are issued back to back.
 *   2. Target.  Straight from the registers of phase 1, the lane that holds frame f of row r
 *      computes limit_peak of the key (or the input), looks the curve of row r up (two LDS reads,
 *      a subtraction and an fmaf) and writes t[f] into row r of the third LDS plane.
 *   3. Walk.  Lane l < R walks row l of that plane: one ds_read_b128 per four frames, issued one
 *      group ahead of its use; per frame a subtraction, a compare, a select of the coefficient and
 *      an fmaf; g[n] is written over t[n], four at a time.  A group that every lane takes whole, or
 *      not at all, runs without per-frame tests; any other group (the last of a row whose count is
 *      no multiple of four) runs the same steps with the test per frame.
 *   4. Apply.  Lanes on consecutive frames again: y = (g * m) * x for both channels from the three
 *      planes, coalesced stores for the frames below the row's count, and the running unsigned
 *      minimum of g's bits for the meter, which is reduced across the wave once, at exit.
 * LDS: plane k (0 target / gain, 1 L, 2 R) row l at (k R + l) TBF_COMP_PITCH floats, PITCH = TILE +
 * 4, behind them curve c at c * TBF_COMP_CURVE_PITCH.  Phases 1, 2 and 4 touch 64 consecutive floats
 * of one row: 64 banks, no conflict.  In the walk lane l reads and writes 16 bytes at float l PITCH
 * + t, banks 4 l + t .. 4 l + t + 3 mod 64: the R lanes that walk (R <= 16 for this pitch) fall on disjoint banks.  The
 * read-ahead is issued by all 64 lanes, outside the test on the group: the 64 - R lanes without a
 * row read row R - 1's address with lane R - 1 (one address, a broadcast, no further bank), use
 * nothing of it and never write.  The
 * curve reads of phase 2 are a gather (neighbouring frames have neighbouring levels only when the
 * signal is slow) and may conflict; they are off the serial lane.
 *
 * Bounds.  Global reads: in[ch][row * inStride + f] and key[ch][row * keyStride + f] with row <
 * nRows and f < count (row) <= frames <= the stride (checked by the host); a frame at or beyond the
 * count reads curves[0] instead.  rows[row], state[row], meters[row], counts[row] with row < nRows;
 * curves[c * 769 + i] with c < nCurves, i < 769.  Global writes: out[ch][row * outStride + f], the
 * same limits with outStride; state[row] and meters[row] with row < nRows.  LDS: planes at (k R + l)
 * PITCH + f with k < 3, l < R; phases 1, 2 and 4 use f < TILE; the walk reads f < TILE + 4 (the
 * read-ahead stops in the row's pad; what it reads there is never used) and writes f < n <= TILE;
 * the curves at 3 R PITCH + c CURVE_PITCH + i with c = rows[row].curve < nCurves (the host's table
 * holds nothing else) and i in [0, 768] (comp_lookup clamps the index before it reads); the launch
 * gives comp_lds_floats (R, nCurves) floats.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbf_comp.h"

/* The tile from frame t0 into registers: load j is source j / (R PER) (L, R, then the key pair),
 * row (j / PER) % R, frame t0 + 64 (j % PER) + lane.  `mine` holds row r's count in lane r, so
 * every count is a uniform value read from that lane. */
template <uint32_t R, bool KEY>
__device__ __forceinline__ void comp_fetch (const tbf_comp_launch& A, uint32_t mine, uint32_t row0, uint32_t t0, uint32_t lane,
                                            float (&v)[(KEY ? 4u : 2u) * R * (TBF_COMP_TILE / TBF_COMP_LANES)])
{
	constexpr uint32_t PER = TBF_COMP_TILE / TBF_COMP_LANES, NS = KEY ? 4u : 2u;
	const float* const idle = A.curves;
#pragma unroll
	for (uint32_t j = 0; j < NS * R * PER; j++) {
		const uint32_t s = j / (R * PER), r = (j / PER) % R;
		const uint32_t f = t0 + (j % PER) * TBF_COMP_LANES + lane;
		const uint32_t n = (uint32_t)__builtin_amdgcn_readlane ((int)mine, (int)r);
		const float*   p = s < 2u ? A.in[s] + (uint64_t)(row0 + r) * A.inStride + f : A.key[s - 2u] + (uint64_t)(row0 + r) * A.keyStride + f;
		v[j]             = *(f < n ? p : idle);
	}
}

template <uint32_t R, bool KEY>
__global__ __launch_bounds__ (TBF_COMP_LANES) void k_comp (tbf_comp_launch A)
{
	constexpr uint32_t PER = TBF_COMP_TILE / TBF_COMP_LANES, NS = KEY ? 4u : 2u, LOADS = NS * R * PER, PL = comp_lds_plane (R);
	extern __shared__ float4 lds4[];
	float* const       tg  = reinterpret_cast<float*> (lds4); /* plane 0; L and R behind it */
	float* const       cur = tg + 3u * PL;

	const uint32_t lane = threadIdx.x, row0 = blockIdx.x * R, row = row0 + lane;
	const bool     own  = lane < R && row < A.nRows;

	/* the counts of the wave's rows (0 beyond the compressor's last and in the lanes without a row) */
	const uint32_t mine = own ? (A.counts ? A.counts[row] : A.frames) : 0u;
	uint32_t       most = mine;
#pragma unroll
	for (int d = 32; d; d >>= 1)
		most = max (most, (uint32_t)__shfl_xor ((int)most, d));

	uint32_t lowest = 0x3F800000u; /* the meter: 1.0f */
	if (most) {
		float    a = 0.0f, r = 0.0f, m = 1.0f, g = 1.0f;
		uint32_t curve = 0u;
		if (own) {
			const tbf_comp_row pr = A.rows[row];
			curve = pr.curve, a = pr.attack, r = pr.release, m = pr.makeup;
			g = A.state[row];
		}
		for (uint32_t i = lane; i < A.nCurves * TBF_COMP_POINTS; i += TBF_COMP_LANES)
			cur[(i / TBF_COMP_POINTS) * TBF_COMP_CURVE_PITCH + i % TBF_COMP_POINTS] = A.curves[i];
		float* const my = tg + min (lane, R - 1u) * TBF_COMP_PITCH; /* lanes without a row never walk */

		uint32_t low[R]; /* row r's smallest gain among this lane's frames */
#pragma unroll
		for (uint32_t k = 0; k < R; k++)
			low[k] = 0x3F800000u;

		float v[LOADS];
		comp_fetch<R, KEY> (A, mine, row0, 0u, lane, v);
		for (uint32_t t0 = 0; t0 < most; t0 += TBF_COMP_TILE) {
			__syncthreads (); /* the curves at the first tile; the tile before is out of the planes */
			/* phases 1 and 2: L and R to their planes, the targets to theirs */
#pragma unroll
			for (uint32_t j = 0; j < R * PER; j++) {
				const uint32_t rr = j / PER, at = rr * TBF_COMP_PITCH + (j % PER) * TBF_COMP_LANES + lane;
				const uint32_t nn = (uint32_t)__builtin_amdgcn_readlane ((int)mine, (int)rr);
				if (t0 + (j % PER) * TBF_COMP_LANES < nn) { /* uniform: the row has a frame in this 64 */
					const float  xl = v[j], xr = v[R * PER + j];
					const float  p  = KEY ? limit_peak (v[2u * R * PER + j], v[3u * R * PER + j]) : limit_peak (xl, xr);
					const uint32_t c = (uint32_t)__builtin_amdgcn_readlane ((int)curve, (int)rr);
					tg[at]           = comp_lookup (cur + c * TBF_COMP_CURVE_PITCH, p);
					tg[PL + at]      = xl;
					tg[2u * PL + at] = xr;
				}
			}
			__syncthreads ();
			if (t0 + TBF_COMP_TILE < most) /* the next one's loads, in flight during the walk */
				comp_fetch<R, KEY> (A, mine, row0, t0 + TBF_COMP_TILE, lane, v);

			/* phase 3, the walk: n frames of this tile are the lane's row's */
			const uint32_t n     = mine > t0 ? min (mine - t0, TBF_COMP_TILE) : 0u;
			const uint32_t steps = min (most - t0, TBF_COMP_TILE);
			if (__any (n != 0u)) {
				float4 nx = *reinterpret_cast<const float4*> (my);
				for (uint32_t t = 0; t < steps; t += TBF_COMP_GROUP) {
					const float4 q = nx;
					nx             = *reinterpret_cast<const float4*> (my + t + TBF_COMP_GROUP); /* at the tile's end: the pad */
					const bool past = t >= n, whole = t + TBF_COMP_GROUP <= n;
					if (__all (past || whole)) {
						if (whole) {
							float4 o;
							o.x = g = comp_step (g, q.x, a, r);
							o.y = g = comp_step (g, q.y, a, r);
							o.z = g = comp_step (g, q.z, a, r);
							o.w = g = comp_step (g, q.w, a, r);
							*reinterpret_cast<float4*> (my + t) = o;
						}
					} else {
						const float x[TBF_COMP_GROUP] = {q.x, q.y, q.z, q.w};
#pragma unroll
						for (uint32_t i = 0; i < TBF_COMP_GROUP; i++)
							if (t + i < n) {
								g         = comp_step (g, x[i], a, r);
								my[t + i] = g;
							}
					}
				}
			}
			__syncthreads ();
			/* phase 4: the gains times the make-up times the staged input, to global memory */
#pragma unroll
			for (uint32_t j = 0; j < R * PER; j++) {
				const uint32_t rr = j / PER, fl = (j % PER) * TBF_COMP_LANES + lane, at = rr * TBF_COMP_PITCH + fl;
				const uint32_t nn = (uint32_t)__builtin_amdgcn_readlane ((int)mine, (int)rr);
				const float    mm = __uint_as_float ((uint32_t)__builtin_amdgcn_readlane ((int)__float_as_uint (m), (int)rr));
				if (t0 + fl < nn) {
					const float    gg  = tg[at];
					const uint64_t o   = (uint64_t)(row0 + rr) * A.outStride + t0 + fl;
					A.out[0][o]        = comp_out (gg, mm, tg[PL + at]);
					A.out[1][o]        = comp_out (gg, mm, tg[2u * PL + at]);
					low[rr]            = min (low[rr], __float_as_uint (gg));
				}
			}
		}
		if (own && mine)
			A.state[row] = g;
		/* row r's minimum over the wave, into lane r */
#pragma unroll
		for (uint32_t k = 0; k < R; k++) {
			uint32_t w = low[k];
#pragma unroll
			for (int d = 32; d; d >>= 1)
				w = min (w, (uint32_t)__shfl_xor ((int)w, d));
			if (lane == k)
				lowest = w;
		}
	}
	if (own && A.meters) {
		tbf_comp_meter mt;
		mt.min_gain   = __uint_as_float (lowest);
		mt.frames     = mine;
		A.meters[row] = mt;
	}
}

extern "C" int tbf_launch_comp (const tbf_comp_launch* A, hipStream_t stream)
{
	if (A->nRows == 0)
		return 0;
	if (!A->in[0] || !A->in[1] || !A->out[0] || !A->out[1] || !A->rows || !A->curves || !A->state || A->nCurves < 1u ||
	    A->nCurves > TBF_COMP_MAX_CURVES || (A->key[0] == nullptr) != (A->key[1] == nullptr))
		return -5;
	constexpr uint32_t R   = TBF_COMP_ROWS;
	const dim3         grid ((A->nRows + R - 1u) / R), block (TBF_COMP_LANES);
	const uint32_t     lds = comp_lds_floats (R, A->nCurves) * 4u;
	if (A->key[0])
		hipLaunchKernelGGL ((k_comp<R, true>), grid, block, lds, stream, *A);
	else
		hipLaunchKernelGGL ((k_comp<R, false>), grid, block, lds, stream, *A);
	return hipGetLastError () == hipSuccess ? 0 : -5;
}
