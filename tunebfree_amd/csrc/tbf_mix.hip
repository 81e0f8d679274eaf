/*
 * tbf_mix.hip -- k_mix, the mixdown stage behind any two float32 planes (tbf_mix_device and the
 * tbf_render_mix* / tbf_process_mix* calls, csrc/tbf_mix.cpp): groups of rows summed into stereo
 * buses through four coefficients per row.
 *
 * The arithmetic is include/tbf.h's definition through mix_term of csrc/tbf_mix.h, which the host
 * restatement runs too.  A bus sample is one serial chain of float32 fmaf over the bus's member
 * rows in ascending row order; the order is part of the definition, so the kernel parallelises
 * over buses and frames and never over one bus's rows, and uses no float atomics.  Nothing
 * depends on the grid: a frame's chain is the same in whichever lane it runs.
 *
 * Pure streaming.  Byte model: 8 B read per member row and valid frame (4 B when L and R are one
 * plane), 8 B written per bus and frame, 24 B of list per member and tile of frames.  The bound is
 * HBM bandwidth: bytes / 6.29 TB/s (the measured copy rate of an MI355X; 8.0 TB/s is the
 * interface's own rate).  The arithmetic is 4 fmaf per 8 B, far below the VALU's rate.
 *
 * The grid is (frame tile, bus); a workgroup is one wave of TBF_MIX_LANES lanes and owns
 * TBF_MIX_LANES x G consecutive frames of one bus, a lane G consecutive ones.  G (4, 2 or 1) is
 * chosen per call by mix_frames_per_lane: 4 when that still gives a couple of thousand waves, fewer
 * otherwise, so that a 128-frame call on one long bus runs in two waves on two CUs rather than in
 * half of one.  That is all the parallelism such a call has: its 128 chains are serial in the
 * rows.
 * The wave walks its bus's member list once, front to back, TBF_MIX_CHUNK members at a time.  A
 * workgroup being one wave, the chunk is staged in the wave's own registers, not in LDS: lane i
 * fetches member i (24 B, the next chunk's while this one is walked), and v_readlane hands the
 * wave member after member as uniform values (the row, the count and the four coefficients live
 * in scalar registers).  A first version staged the chunk in LDS; its ds_read and wait per
 * member and value made the issue of a member's loads cost more than the loads (DESIGN.md
 * section 4.12).  A member whose count ends before the tile is skipped by the whole wave and none
 * of its samples is read.
 * Loads: U = TBF_MIX_LOADS / (2 G) members are loaded before the first of them is used, so 32
 * dwords per lane (8 KiB per wave) are in flight whatever G is; the fmaf chain behind them is
 * serial per frame, the loads are not.  A member's loads are one dwordx4 (G = 4) or dwordx2
 * (G = 2) per plane when both of that row's addresses are aligned to the load and the lane's
 * group lies within the row's count -- the tbf_render_device contract allows any float alignment
 * and odd strides, so this is decided per member row -- and dwords otherwise, each under its own
 * j < count.
 * Stores: one dwordx4 / dwordx2 per plane when the bus's output row is aligned and the group lies
 * within `frames`, dwords otherwise and at the tail.  Nothing outside [0, frames) of an output
 * row is written.  A bus without members, and frames none of its members reaches, get +0.0f.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbf_mix.h"

template <int G>
struct mix_vec;
template <>
struct mix_vec<4> {
	typedef float4 type;
};
template <>
struct mix_vec<2> {
	typedef float2 type;
};
template <>
struct mix_vec<1> {
	typedef float type;
};

/* lane i's value of v, the same in every lane (i is uniform) */
__device__ __forceinline__ uint32_t mix_lane (uint32_t v, uint32_t i) { return (uint32_t)__builtin_amdgcn_readlane ((int)v, (int)i); }
__device__ __forceinline__ float    mix_lane (float v, uint32_t i) { return __uint_as_float (mix_lane (__float_as_uint (v), i)); }

template <int G>
__global__ __launch_bounds__ (TBF_MIX_LANES) void k_mix (tbf_mix_launch P)
{
	constexpr int      U = (int)TBF_MIX_LOADS / (2 * G); /* members in flight */
	typedef typename mix_vec<G>::type vec;

	const uint32_t bus = P.busBase + blockIdx.y, lane = threadIdx.x;
	const uint64_t t0 = (uint64_t)blockIdx.x * (TBF_MIX_LANES * G); /* the tile's first frame, < frames */
	const uint64_t j  = t0 + (uint64_t)lane * G;                     /* the lane's first frame */
	const uint32_t m0 = P.busOff[bus], m1 = P.busOff[bus + 1];

	float accL[G], accR[G];
#pragma unroll
	for (int k = 0; k < G; k++)
		accL[k] = accR[k] = 0.0f;

	/* lane i's member of the chunk that starts at c: an entry of the list, or nothing behind its end */
	auto fetch = [&] (uint32_t c) {
		tbf_mix_member m = {0u, 0u, 0.0f, 0.0f, 0.0f, 0.0f};
		if (c < m1 && lane < m1 - c)
			m = P.members[c + lane];
		return m;
	};
	tbf_mix_member next = fetch (m0);
	for (uint32_t c0 = m0; c0 < m1; c0 += TBF_MIX_CHUNK) {
		const uint32_t       nc  = min (TBF_MIX_CHUNK, m1 - c0);
		const tbf_mix_member cur = next;
		next                     = fetch (c0 + TBF_MIX_CHUNK); /* under way while this chunk is walked */
		const uint32_t       curCnt = min (cur.count, P.frames);
		for (uint32_t u0 = 0; u0 < nc; u0 += U) {
			float    xl[U][G], xr[U][G]; /* set and used under the same j + k < cnt[u] */
			uint32_t cnt[U];
			/* the loads of up to U members, all issued before the first use */
#pragma unroll
			for (int u = 0; u < U; u++) {
				const uint32_t i = min (u0 + u, TBF_MIX_CHUNK - 1u);
				cnt[u]           = u0 + u < nc ? mix_lane (curCnt, i) : 0u;
				if (cnt[u] <= t0) /* uniform: no such member, or it ends before this tile */
					continue;
				const uint64_t row = mix_lane (cur.row, i);
				const float* __restrict__ pl = P.in[0] + row * P.inStride;
				const float* __restrict__ pr = P.in[1] + row * P.inStride;
				const bool wide = G > 1 && ((((uintptr_t)pl | (uintptr_t)pr) & (4u * G - 1u)) == 0);
				if (wide && j + G <= cnt[u]) {
					const vec a = *reinterpret_cast<const vec*> (pl + j), b = *reinterpret_cast<const vec*> (pr + j);
					__builtin_memcpy (xl[u], &a, sizeof (vec));
					__builtin_memcpy (xr[u], &b, sizeof (vec));
				} else {
#pragma unroll
					for (int k = 0; k < G; k++)
						if (j + k < cnt[u]) {
							xl[u][k] = pl[j + k];
							xr[u][k] = pr[j + k];
						}
				}
			}
			/* their terms, in the list's order */
#pragma unroll
			for (int u = 0; u < U; u++) {
				if (cnt[u] <= t0)
					continue;
				const uint32_t i  = min (u0 + u, TBF_MIX_CHUNK - 1u);
				const float    ll = mix_lane (cur.ll, i), lr = mix_lane (cur.lr, i);
				const float    rl = mix_lane (cur.rl, i), rr = mix_lane (cur.rr, i);
#pragma unroll
				for (int k = 0; k < G; k++)
					if (j + k < cnt[u])
						mix_term (ll, lr, rl, rr, xl[u][k], xr[u][k], accL[k], accR[k]);
			}
		}
	}

	if (j >= P.frames)
		return;
	float* const ol = P.out[0] + (uint64_t)bus * P.outStride;
	float* const orr = P.out[1] + (uint64_t)bus * P.outStride;
	const bool   wide = G > 1 && ((((uintptr_t)ol | (uintptr_t)orr) & (4u * G - 1u)) == 0);
	if (wide && j + G <= P.frames) {
		vec a, b;
		__builtin_memcpy (&a, accL, sizeof (vec));
		__builtin_memcpy (&b, accR, sizeof (vec));
		*reinterpret_cast<vec*> (ol + j)  = a;
		*reinterpret_cast<vec*> (orr + j) = b;
	} else {
#pragma unroll
		for (int k = 0; k < G; k++)
			if (j + k < P.frames) {
				ol[j + k]  = accL[k];
				orr[j + k] = accR[k];
			}
	}
}

template <int G>
static int mix_launch (const tbf_mix_launch& P, hipStream_t stream)
{
	const uint64_t tile  = (uint64_t)TBF_MIX_LANES * G;
	const uint32_t tiles = (uint32_t)(((uint64_t)P.frames + tile - 1) / tile);
	hipLaunchKernelGGL ((k_mix<G>), dim3 (tiles, P.nBuses), dim3 (TBF_MIX_LANES), 0, stream, P);
	return hipGetLastError () == hipSuccess ? 0 : -5;
}

extern "C" int tbf_launch_mix (const tbf_mix_launch* P, hipStream_t stream)
{
	if (P->nBuses == 0 || P->frames == 0)
		return 0;
	if (P->nBuses > TBF_MIX_MAX_BUSES || !P->busOff || !P->out[0] || !P->out[1])
		return -5;
	switch (P->group) {
	case 4:
		return mix_launch<4> (*P, stream);
	case 2:
		return mix_launch<2> (*P, stream);
	case 1:
		return mix_launch<1> (*P, stream);
	}
	return -5;
}
