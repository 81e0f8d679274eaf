/*
 * tbf_limit_tp.hip -- k_limit_tp, the bus limiter with a true-peak detector (tbf_limiter_create_tp,
 * csrc/tbf_limit.cpp): k_limit's gain law on a per-frame peak that is the largest magnitude of the
 * samples E = 6 frames back and of the F - 1 (F = 2) or 4 (F = 4) interpolated values of the
 * true-peak meter's chains, applied to the input D + E = A + 5 frames late.
 *
 * The arithmetic is include/tbf.h's definition through limit_tp_peak, limit_target and limit_out of
 * csrc/tbf_limit.h and tpeak_y of csrc/tbf_tpeak.h, which the host restatement runs too.  k_limit
 * (csrc/tbf_limit.hip) is left as it is: this file restates its later phases (minimum, sum, write,
 * meters, and the meters' preset kernel) and shares only the header, so the plain limiter's
 * instructions do not move.  The two copies are tied by nothing but this note and the one in
 * csrc/tbf_limit.hip: a fix to either belongs in both.
 *
 * The grid, the tile and the two float arrays are k_limit's: (frame tile, row), limit_tile (A, H)
 * output frames per workgroup, t of the tile and of the Hn = 2 A + H - 2 frames in front of it in
 * LDS.  Only the staging differs:
 *   Stage.  t[f] needs both channels' frames f - 11 .. f.  The staged frames are taken a pass of
 * the workgroup at a time (TBF_LIMIT_SUB = 1024 frames): the raw samples of the pass and of the 11
 * frames in front of it go to a third LDS region of 2 x TBF_LIMIT_TP_RAW floats (dword loads,
 * coalesced; from the row's history where the frame lies before the call, +0.0f at or beyond the
 * count), then lane l reads its 16-float window of either channel as four aligned 16-byte values,
 * as k_tpeak does, evaluates 4 frames x 2 channels x F chains of 12 v_fma_f32 in tap order with the
 * coefficients as literals, and stores four t as one 16-byte value.  Two barriers a pass.  The raw
 * region is small and fixed, so the LDS is k_limit's plus 8288 B: 65696 B at (512, 4096), two
 * workgroups a CU; 17568 B at (64, 0).
 *   Next history.  The last Hn_tp = Hn + 11 frames of (history, input), written by the load that
 * owns the frame: every tile the input frames of its own, tile 0 the part that is still the old
 * history.  The 11 frames in front of a later pass were the body of the pass before and are not
 * written again.  Two sides as in k_limit, so no tile reads what another writes.
 *   Minimum, sum, write, meters: k_limit's, with the delayed input read D + E back.
 *
 * Arithmetic per output frame: (1 + Hn / tile) x 24 F fmaf for the chains
 * (the halo's t is recomputed by every tile), A adds for the sum.  Bytes as k_limit, with Hn_tp in
 * place of Hn.
 *
 * Bounds.  Global reads: x[f] with 0 <= f < count <= frames <= inStride (checked by the host);
 * the old history at Hn_tp + f with -Hn_tp <= f < 0: the first staged frame is t0 - Hn and the
 * raw halo reaches 11 further, and the delayed read goes D + E = A + 5 <= Hn_tp back.  The new
 * history at f - h0 with h0 = count - Hn_tp <= f < count.  LDS: t at base + 4 lane + {0..3} only
 * where base + 4 lane < N, and N + 3 < limit_lds_floats; raw words 12 + k 256 + lane < 1036 and
 * lane < 12; the window's words 4 lane .. 4 lane + 15 <= 1035.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbf_limit.h"

extern __shared__ float4 limit_tp_lds[];

#define LIMIT_TP_LOADS (TBF_LIMIT_SUB / TBF_LIMIT_LANES) /* dwords a lane loads per channel and pass */
#define TBF_LIMIT_TP_MAX_DEVICES 64u /* devices whose LDS grant is remembered; beyond, every launch asks */

__global__ __launch_bounds__ (TBF_LIMIT_LANES) void k_limit_tp_meters (tbf_limit_meter* m, uint32_t n)
{
	const uint32_t r = blockIdx.x * TBF_LIMIT_LANES + threadIdx.x;
	if (r < n) {
		m[r].min_gain = 1.0f;
		m[r].reduced  = 0u;
		m[r].clamped  = 0u;
	}
}

template <uint32_t F> __global__ __launch_bounds__ (TBF_LIMIT_LANES) void k_limit_tp (tbf_limit_launch P)
{
	const uint32_t      row = P.rowBase + blockIdx.y, lane = threadIdx.x;
	const tbf_limit_row rw  = P.rows[row];
	const uint32_t      cnt = rw.count;
	const uint32_t      A = P.ahead, W = A + P.hold, Hn = limit_history (A, P.hold);
	const uint32_t      Ht = limit_tp_history (A, P.hold), DE = A - 1u + TBF_LIMIT_TP_DELAY;
	const uint32_t      tile = limit_tile (A, P.hold);
	const int64_t       t0   = (int64_t)blockIdx.x * tile; /* the tile's first frame */
	if (t0 >= (int64_t)cnt)
		return;
	const float    c  = P.ceiling;
	const uint32_t N  = tile + Hn;                       /* staged t: frames t0 - Hn .. t0 + tile - 1 */
	const uint32_t NF = limit_lds_floats (A, P.hold);
	float*         src = reinterpret_cast<float*> (limit_tp_lds);
	float*         dst = src + NF;
	float* const   raw = dst + NF;                       /* [channel][TBF_LIMIT_TP_RAW] */

	const float* __restrict__ xl = P.in[0] + (uint64_t)row * P.inStride;
	const float* __restrict__ xr = P.in[1] + (uint64_t)row * P.inStride;
	float* const        hrow = P.hist + (uint64_t)row * 4u * Ht;
	const float* const  hOldL = hrow + (uint64_t)(2u * rw.side) * Ht, * const hOldR = hOldL + Ht;
	float* const        hNewL = hrow + (uint64_t)(2u * (rw.side ^ 1u)) * Ht, * const hNewR = hNewL + Ht;
	const int64_t       h0 = (int64_t)cnt - (int64_t)Ht;   /* the frame that becomes the next history's first */

	/* stage t a pass at a time, and the next history */
	for (uint32_t base = 0; base < N; base += TBF_LIMIT_SUB) {
		const int64_t fb = t0 - (int64_t)Hn + base; /* the frame of staged index base */
		float         vl[LIMIT_TP_LOADS], vr[LIMIT_TP_LOADS], hl = 0.0f, hr = 0.0f;
#pragma unroll
		for (uint32_t k = 0; k < LIMIT_TP_LOADS; k++) {
			const uint32_t i = base + k * TBF_LIMIT_LANES + lane;
			const int64_t  f = fb + k * TBF_LIMIT_LANES + lane;
			vl[k] = vr[k] = 0.0f;
			if (i < N && f < (int64_t)cnt) {
				if (f < 0) {
					vl[k] = hOldL[(int64_t)Ht + f];
					vr[k] = hOldR[(int64_t)Ht + f];
				} else {
					vl[k] = xl[f];
					vr[k] = xr[f];
				}
				if (f >= h0 && (f >= t0 || blockIdx.x == 0)) {
					hNewL[f - h0] = vl[k];
					hNewR[f - h0] = vr[k];
				}
			}
		}
		if (lane >= 1u && lane < TBF_LIMIT_TP_HALO) {
			const int64_t f = fb - (int64_t)TBF_LIMIT_TP_HALO + lane; /* at least t0 - Hn_tp; a later pass may begin beyond count */
			if (f < 0) {
				hl = hOldL[(int64_t)Ht + f];
				hr = hOldR[(int64_t)Ht + f];
			} else if (f < (int64_t)cnt) {
				hl = xl[f];
				hr = xr[f];
			}
			if (base == 0 && f >= h0 && blockIdx.x == 0) { /* frames before t0: tile 0's, all of them old history */
				hNewL[f - h0] = hl;
				hNewR[f - h0] = hr;
			}
		}
#pragma unroll
		for (uint32_t k = 0; k < LIMIT_TP_LOADS; k++) {
			raw[TBF_LIMIT_TP_HALO + k * TBF_LIMIT_LANES + lane]                    = vl[k];
			raw[TBF_LIMIT_TP_RAW + TBF_LIMIT_TP_HALO + k * TBF_LIMIT_LANES + lane] = vr[k];
		}
		if (lane < TBF_LIMIT_TP_HALO) {
			raw[lane]                    = hl;
			raw[TBF_LIMIT_TP_RAW + lane] = hr;
		}
		__syncthreads ();

		const uint32_t i0 = base + TBF_LIMIT_GROUP * lane; /* the lane's first staged index of this pass */
		if (i0 < N) {
			const float4* const ql = reinterpret_cast<const float4*> (raw + TBF_LIMIT_GROUP * lane);
			const float4* const qr = reinterpret_cast<const float4*> (raw + TBF_LIMIT_TP_RAW + TBF_LIMIT_GROUP * lane);
			const float4        a = ql[0], b = ql[1], d = ql[2], e = ql[3];
			const float4        s = qr[0], u = qr[1], v = qr[2], w = qr[3];
			const float wl[16] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, d.x, d.y, d.z, d.w, e.x, e.y, e.z, e.w};
			const float wr[16] = {s.x, s.y, s.z, s.w, u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w, w.x, w.y, w.z, w.w};
			float       tv[TBF_LIMIT_GROUP];
#pragma unroll
			for (uint32_t k = 0; k < TBF_LIMIT_GROUP; k++) {
				const float p = limit_tp_peak (F, &wl[TBF_LIMIT_TP_HALO + k], &wr[TBF_LIMIT_TP_HALO + k]);
				tv[k]         = fb + (int64_t)(TBF_LIMIT_GROUP * lane + k) < (int64_t)cnt ? limit_target (p, c) : 1.0f;
			}
			*reinterpret_cast<float4*> (src + i0) = make_float4 (tv[0], tv[1], tv[2], tv[3]);
		}
		__syncthreads (); /* the next pass rewrites raw; the last one's is the barrier in front of the minima */
	}

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
				const int64_t fd = n + k - (int64_t)DE;
				const float   a  = fd < 0 ? hOldL[(int64_t)Ht + fd] : xl[fd];
				const float   b  = fd < 0 ? hOldR[(int64_t)Ht + fd] : xr[fd];
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

template <uint32_t F> static int launchTp (const tbf_limit_launch* P, dim3 grid, uint32_t lds, hipStream_t stream)
{
	/* Only a launch that needs more dynamic LDS than every launch may have asks for it, and only
	 * when it needs more than was asked for before: the attribute is the kernel's, so once per
	 * size and device, not per call.  (A second thread may ask again; the call is idempotent.) */
	static uint32_t granted[TBF_LIMIT_TP_MAX_DEVICES];
	int             dev = 0;
	if (lds > 48u * 1024u) {
		if (hipGetDevice (&dev) != hipSuccess || dev < 0)
			return -5;
		if (dev >= (int)TBF_LIMIT_TP_MAX_DEVICES || granted[dev] < lds) {
			if (hipFuncSetAttribute (reinterpret_cast<const void*> (&k_limit_tp<F>), hipFuncAttributeMaxDynamicSharedMemorySize,
			                         (int)lds) != hipSuccess)
				return -5;
			if (dev < (int)TBF_LIMIT_TP_MAX_DEVICES)
				granted[dev] = lds;
		}
	}
	hipLaunchKernelGGL (k_limit_tp<F>, grid, dim3 (TBF_LIMIT_LANES), lds, stream, *P);
	return 0;
}

/* P->hist is [row][side][channel][Hn_tp]; F is 2 or 4 */
extern "C" int tbf_launch_limit_tp (const tbf_limit_launch* P, uint32_t F, hipStream_t stream)
{
	if (P->nRows == 0)
		return 0;
	if (P->nRows > TBF_LIMIT_MAX_ROWS || !P->rows || !P->hist || !P->out[0] || !P->out[1] || (F != 2u && F != 4u))
		return -5;
	if (P->meters)
		hipLaunchKernelGGL (k_limit_tp_meters, dim3 ((P->nRows + TBF_LIMIT_LANES - 1u) / TBF_LIMIT_LANES), dim3 (TBF_LIMIT_LANES), 0,
		                    stream, P->meters + P->rowBase, P->nRows);
	if (P->maxCount) {
		const uint32_t tile  = limit_tile (P->ahead, P->hold);
		const uint32_t tiles = (uint32_t)(((uint64_t)P->maxCount + tile - 1u) / tile);
		const uint32_t lds   = limit_tp_lds_bytes (P->ahead, P->hold);
		const dim3     grid (tiles, P->nRows);
		if (F == 4u ? launchTp<4u> (P, grid, lds, stream) : launchTp<2u> (P, grid, lds, stream))
			return -5;
	}
	return hipGetLastError () == hipSuccess ? 0 : -5;
}
