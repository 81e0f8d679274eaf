/*
 * tbf_limit.hip -- k_limit, the look-ahead peak limiter behind any two float32 planes
 * (tbf_limit_device, csrc/tbf_limit.cpp): per row a gain that is the mean over A frames of the
 * minimum over W = A + H frames of the per-frame target c / peak, applied to the input D = A - 1
 * frames late and clamped to the ceiling.
 *
 * The arithmetic is include/tbf.h's definition through limit_peak, limit_target and limit_out of
 * csrc/tbf_limit.h, which the host restatement runs too.  The window minimum is exact in any
 * order; the gain's sum is not, so every frame's sum is the literal chain of A float32 adds in
 * ascending order from +0.0f: no running sum, no tree, no re-association.
 *
 * Byte model: 16 B per frame (8 B read, 8 B written), plus per tile the halo's 8 B x Hn
 * (Hn = 2 A + H - 2 frames in front of the tile, which the neighbouring tile has just read) and
 * the delayed input's second read, both served by L2, plus 8 B per frame of the row's last Hn
 * written as its next history.  Arithmetic: A adds per frame in the sum, 2 log2 (W) + 2 LDS
 * accesses per staged frame for the minimum, one division per staged frame.  The bound is
 * bytes / 6.29 TB/s (the measured copy rate of an MI355X) for a short A and the VALU's rate of
 * float32 adds beyond (DESIGN.md section 4.13 has the figures).
 *
 * The grid is (frame tile, row); a workgroup of TBF_LIMIT_LANES lanes owns limit_tile (A, H)
 * consecutive output frames of one row.  A tile at or beyond its row's count exits.
 *   Stage.  t of the tile and of the Hn frames in front of it goes to LDS, recomputed from the raw
 * samples: from the row's history where the halo reaches before the call, from the input
 * otherwise.  The state is raw input only.  The same pass writes the row's next history, the last
 * Hn frames of (history, input): every tile the input frames it owns, tile 0 the part that is
 * still the old history when the call is shorter than Hn.  A row has two history buffers; the
 * call reads tbf_limit_row.side and writes the other, so no tile reads what another writes, and
 * the host flips the side of every row that took frames.
 *   Minimum.  Doubling between two LDS arrays: after pass k, M[i] = min t[i - 2^k + 1 .. i];
 * m = min (M[i], M[i - (W - 2^k)]) with 2^k <= W < 2^(k+1).  m is stored so that a lane's first
 * frame sits on a 16-byte boundary.
 *   Sum.  A lane carries TBF_LIMIT_GROUP = 4 consecutive frames.  Their four windows overlap in
 * all but three terms each side, so the lane reads m once, a ds_read_b128 per four terms, and
 * feeds four accumulators: the LDS reads are shared, the adds are not.
 *   Write.  g x the delayed input, clamped; one dwordx4 per plane when both of the row's output
 * addresses are 16-byte aligned and the group lies within the count (the tbf_render_device
 * contract allows any float alignment and odd strides, so this is decided per row), dwords
 * otherwise and at the tail.  Nothing outside [0, count) of an output row is written.
 *   Meters.  min_gain as the bits of a non-negative float (which order as the floats do), reduced
 * and clamped as counts: reduced over the wave with shuffles, then one integer atomicMin and two
 * integer atomicAdd per wave, skipped when they would change nothing.  Integer minima and sums
 * do not depend on order, so the meters are exact.  k_limit_meters sets them to {1.0f, 0, 0} in
 * front of k_limit on the same stream.
 *
 * k_limit_tp (csrc/tbf_limit_tp.hip, the limiter with a true-peak detector) restates the minimum,
 * the sum, the write and the meters of this file word for word, so that this kernel's
 * instructions stay as they are: a fix to either copy belongs in both.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbf_limit.h"

extern __shared__ float4 limit_lds[];

__global__ __launch_bounds__ (TBF_LIMIT_LANES) void k_limit_meters (tbf_limit_meter* m, uint32_t n)
{
	const uint32_t r = blockIdx.x * TBF_LIMIT_LANES + threadIdx.x;
	if (r < n) {
		m[r].min_gain = 1.0f;
		m[r].reduced  = 0u;
		m[r].clamped  = 0u;
	}
}

__global__ __launch_bounds__ (TBF_LIMIT_LANES) void k_limit (tbf_limit_launch P)
{
	const uint32_t      row = P.rowBase + blockIdx.y, lane = threadIdx.x;
	const tbf_limit_row rw  = P.rows[row];
	const uint32_t      cnt = rw.count;
	const uint32_t      A = P.ahead, W = A + P.hold, Hn = limit_history (A, P.hold), D = A - 1u;
	const uint32_t      tile = limit_tile (A, P.hold);
	const int64_t       t0   = (int64_t)blockIdx.x * tile; /* the tile's first frame */
	if (t0 >= (int64_t)cnt)
		return;
	const float    c  = P.ceiling;
	const uint32_t N  = tile + Hn;                       /* staged frames: t0 - Hn .. t0 + tile - 1 */
	const uint32_t NF = limit_lds_floats (A, P.hold);
	float*         src = reinterpret_cast<float*> (limit_lds);
	float*         dst = src + NF;

	const float* __restrict__ xl = P.in[0] + (uint64_t)row * P.inStride;
	const float* __restrict__ xr = P.in[1] + (uint64_t)row * P.inStride;
	float* const        hrow = P.hist + (uint64_t)row * 4u * Hn;
	const float* const  hOldL = hrow + (uint64_t)(2u * rw.side) * Hn, * const hOldR = hOldL + Hn;
	float* const        hNewL = hrow + (uint64_t)(2u * (rw.side ^ 1u)) * Hn, * const hNewR = hNewL + Hn;
	const int64_t       h0 = (int64_t)cnt - (int64_t)Hn;   /* the frame that becomes the next history's first */

	/* stage t, and the next history */
	for (uint32_t i = lane; i < N; i += TBF_LIMIT_LANES) {
		const int64_t f = t0 - (int64_t)Hn + i;
		float         tv = 1.0f;
		if (f < (int64_t)cnt) {
			float a, b;
			if (f < 0) {
				a = hOldL[(int64_t)Hn + f];
				b = hOldR[(int64_t)Hn + f];
			} else {
				a = xl[f];
				b = xr[f];
			}
			tv = limit_target (limit_peak (a, b), c);
			if (f >= h0 && (f >= t0 || blockIdx.x == 0)) {
				hNewL[f - h0] = a;
				hNewR[f - h0] = b;
			}
		}
		src[i] = tv;
	}
	__syncthreads ();

	/* window minima by doubling */
	uint32_t s = 1u;
	while (2u * s <= W) {
		for (uint32_t i = lane; i < N; i += TBF_LIMIT_LANES) {
			float v = src[i];
			if (i >= s) {
				const float u = src[i - s];
				v             = u < v ? u : v;
			}
			dst[i] = v;
		}
		__syncthreads ();
		float* const x = src;
		src            = dst;
		dst            = x;
		s *= 2u;
	}
	/* m of frame t0 - A + 1 + k, k < tile + A - 1, to dst[AO - A + 1 + k]: frame t0 at dst[AO] */
	const uint32_t AO = A < 4u ? 4u : A;
	for (uint32_t k = lane; k < tile + A - 1u; k += TBF_LIMIT_LANES) {
		const uint32_t i = W - 1u + k;
		const float    u = src[i - (W - s)], v = src[i];
		dst[AO - A + 1u + k] = u < v ? u : v;
	}
	__syncthreads ();

	const float  inv  = 1.0f / (float)A;
	float* const ol   = P.out[0] + (uint64_t)row * P.outStride;
	float* const orr  = P.out[1] + (uint64_t)row * P.outStride;
	const bool   wide = ((((uintptr_t)ol | (uintptr_t)orr) & 15u) == 0);
	uint32_t     minG = 0x3f800000u, reduced = 0u, clamped = 0u;

	for (uint32_t q = lane * TBF_LIMIT_GROUP; q < tile; q += TBF_LIMIT_SUB) {
		const int64_t n = t0 + q; /* the lane's first frame of this pass */
		if (n >= (int64_t)cnt)
			break;
		float acc[TBF_LIMIT_GROUP] = {0.0f, 0.0f, 0.0f, 0.0f};
		if (A >= 4u) {
			/* dst[q + 4 g + e] is m of frame n - A + 4 g + e; frame n + k sums n + k - A + 1 .. n + k */
			const float4* const mp = reinterpret_cast<const float4*> (dst + q);
			float4              v  = mp[0];
			acc[0] = acc[0] + v.y, acc[0] = acc[0] + v.z, acc[0] = acc[0] + v.w;
			acc[1] = acc[1] + v.z, acc[1] = acc[1] + v.w;
			acc[2] = acc[2] + v.w;
			const uint32_t G  = A / 4u;
			float4         nx = mp[1]; /* the next four terms are under way while these are added */
			for (uint32_t g = 1; g < G; g++) {
				v  = nx;
				nx = mp[g + 1u];
#pragma unroll
				for (int k = 0; k < (int)TBF_LIMIT_GROUP; k++) {
					acc[k] = acc[k] + v.x;
					acc[k] = acc[k] + v.y;
					acc[k] = acc[k] + v.z;
					acc[k] = acc[k] + v.w;
				}
			}
			v = nx; /* mp[G] */
			acc[0] = acc[0] + v.x;
			acc[1] = acc[1] + v.x, acc[1] = acc[1] + v.y;
			acc[2] = acc[2] + v.x, acc[2] = acc[2] + v.y, acc[2] = acc[2] + v.z;
			acc[3] = acc[3] + v.x, acc[3] = acc[3] + v.y, acc[3] = acc[3] + v.z, acc[3] = acc[3] + v.w;
		} else {
#pragma unroll
			for (int k = 0; k < (int)TBF_LIMIT_GROUP; k++)
				for (uint32_t j = 0; j < A; j++)
					acc[k] = acc[k] + dst[q + AO + k - A + 1u + j];
		}

		float yl[TBF_LIMIT_GROUP], yr[TBF_LIMIT_GROUP];
#pragma unroll
		for (int k = 0; k < (int)TBF_LIMIT_GROUP; k++) {
			yl[k] = yr[k] = 0.0f;
			if (n + k < (int64_t)cnt) {
				const float   g  = acc[k] * inv;
				const int64_t fd = n + k - (int64_t)D;
				const float   a  = fd < 0 ? hOldL[(int64_t)Hn + fd] : xl[fd];
				const float   b  = fd < 0 ? hOldR[(int64_t)Hn + fd] : xr[fd];
				yl[k]            = limit_out (g, a, c, clamped);
				yr[k]            = limit_out (g, b, c, clamped);
				minG             = min (minG, __float_as_uint (g));
				reduced += g < 1.0f ? 1u : 0u;
			}
		}
		if (wide && n + (int64_t)TBF_LIMIT_GROUP <= (int64_t)cnt) {
			*reinterpret_cast<float4*> (ol + n)  = make_float4 (yl[0], yl[1], yl[2], yl[3]);
			*reinterpret_cast<float4*> (orr + n) = make_float4 (yr[0], yr[1], yr[2], yr[3]);
		} else {
#pragma unroll
			for (int k = 0; k < (int)TBF_LIMIT_GROUP; k++)
				if (n + k < (int64_t)cnt) {
					ol[n + k]  = yl[k];
					orr[n + k] = yr[k];
				}
		}
	}

	if (P.meters) { /* uniform over the launch: every lane of the wave takes part, idle ones with nothing */
#pragma unroll
		for (int d = 32; d; d >>= 1) {
			minG = min (minG, (uint32_t)__shfl_xor ((int)minG, d));
			reduced += (uint32_t)__shfl_xor ((int)reduced, d);
			clamped += (uint32_t)__shfl_xor ((int)clamped, d);
		}
		if ((lane & 63u) == 0) {
			tbf_limit_meter* const t = P.meters + row;
			if (minG < 0x3f800000u)
				atomicMin (reinterpret_cast<unsigned int*> (&t->min_gain), minG);
			if (reduced)
				atomicAdd (&t->reduced, reduced);
			if (clamped)
				atomicAdd (&t->clamped, clamped);
		}
	}
}

extern "C" int tbf_launch_limit (const tbf_limit_launch* P, hipStream_t stream)
{
	if (P->nRows == 0)
		return 0;
	if (P->nRows > TBF_LIMIT_MAX_ROWS || !P->rows || !P->hist || !P->out[0] || !P->out[1])
		return -5;
	if (P->meters)
		hipLaunchKernelGGL (k_limit_meters, dim3 ((P->nRows + TBF_LIMIT_LANES - 1u) / TBF_LIMIT_LANES), dim3 (TBF_LIMIT_LANES), 0,
		                    stream, P->meters + P->rowBase, P->nRows);
	if (P->maxCount) {
		const uint32_t tile  = limit_tile (P->ahead, P->hold);
		const uint32_t tiles = (uint32_t)(((uint64_t)P->maxCount + tile - 1u) / tile);
		const size_t   lds   = 2u * (size_t)limit_lds_floats (P->ahead, P->hold) * sizeof (float);
		hipLaunchKernelGGL (k_limit, dim3 (tiles, P->nRows), dim3 (TBF_LIMIT_LANES), lds, stream, *P);
	}
	return hipGetLastError () == hipSuccess ? 0 : -5;
}
