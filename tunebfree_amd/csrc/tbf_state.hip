/*
 * tbf_state.hip -- k_state_move, the batched mover of per-instance device state
 * (tbf_instances_clone / tbf_instances_save / tbf_instances_load, csrc/tbf_fork.cpp).
 *
 * An instance's device state is a handful of arrays, each contiguous per instance (st,
 * wring, rslab, tgc, the persistent program slots).  One launch moves, for every (source,
 * destination) pair of a list, every segment of a short table from the source's instance of
 * the array to the destination's: array to array for a clone, array to packed record for a
 * save, packed record to array for a load (a record is a segment table whose bases are
 * offsets into one staging buffer and whose stride is the record length).
 *
 * Grid: x = the slices of all segments (a slice is 256 lanes x U loads of the segment's
 * width), y = the pairs; so one pair (about 350 KB) and 4096 pairs both spread over the chip.
 * The host picks each segment's width (16 B where base, strides and length allow, else 8 B)
 * and U; a lane issues its U loads before its first store, and a load or store is made only
 * where its whole element lies inside the instance's segment, so nothing outside it is read
 * or written.  A source read by many pairs needs nothing special: reads do not conflict.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbf_state.h"

#define SM_THREADS 256

/* native vectors (HIP's uint4 is a struct: copying one is a memcpy, which the compiler sinks
 * to its store, so the loads would not stay ahead of the stores) */
typedef uint32_t u32x4 __attribute__ ((ext_vector_type (4)));
typedef uint32_t u32x2 __attribute__ ((ext_vector_type (2)));

template <typename V, int U>
__device__ __forceinline__ void move_slice (const unsigned char* __restrict__ s, unsigned char* __restrict__ d,
                                            uint64_t first, uint64_t bytes)
{
	V        v[U];
	uint64_t off[U];
#pragma unroll
	for (int j = 0; j < U; j++)
		off[j] = first + ((uint64_t)j * SM_THREADS + threadIdx.x) * sizeof (V);
	if (first + (uint64_t)U * SM_THREADS * sizeof (V) <= bytes) {
		/* a whole slice (uniform over the workgroup): the U loads, then the U stores, no guards */
#pragma unroll
		for (int j = 0; j < U; j++)
			v[j] = *reinterpret_cast<const V*> (s + off[j]);
#pragma unroll
		for (int j = 0; j < U; j++)
			*reinterpret_cast<V*> (d + off[j]) = v[j];
		return;
	}
	/* the segment's last slice: an element only where it lies inside (bytes is a multiple of
	 * sizeof (V), so an element that starts inside ends inside) */
#pragma unroll
	for (int j = 0; j < U; j++)
		if (off[j] < bytes)
			v[j] = *reinterpret_cast<const V*> (s + off[j]);
#pragma unroll
	for (int j = 0; j < U; j++)
		if (off[j] < bytes)
			*reinterpret_cast<V*> (d + off[j]) = v[j];
}

template <int U>
__global__ __launch_bounds__ (SM_THREADS) void k_state_move (tbf_move_table T, const uint32_t* __restrict__ pairSrc,
                                                             const uint32_t* __restrict__ pairDst)
{
	/* the segment of this slice (nseg <= TBF_MOVE_SEGS: a scan of uniform values) */
	uint32_t g = 0;
	while (g + 1 < T.nseg && blockIdx.x >= T.seg[g + 1].slice0)
		g++;
	const tbf_move_seg& S  = T.seg[g];
	const uint32_t      sl = blockIdx.x - S.slice0;
	const uint64_t      si = pairSrc[blockIdx.y], di = pairDst[blockIdx.y];
	const unsigned char* s = S.src + si * S.srcStride;
	unsigned char*       d = S.dst + di * S.dstStride;
	if (S.wide)
		move_slice<u32x4, U> (s, d, (uint64_t)sl * SM_THREADS * U * sizeof (u32x4), S.bytes);
	else
		move_slice<u32x2, U> (s, d, (uint64_t)sl * SM_THREADS * U * sizeof (u32x2), S.bytes);
}

/* Fills the table's slice ranges for U loads per lane and launches; segments of zero bytes
 * are skipped.  Every base, stride and length must be a multiple of 8 (16 where wide). */
extern "C" int tbf_launch_state_move (tbf_move_table* T, const uint32_t* dPairSrc, const uint32_t* dPairDst,
                                      uint32_t npairs, uint32_t unroll, hipStream_t stream)
{
	if (npairs == 0 || T->nseg == 0)
		return 0;
	if (T->nseg > TBF_MOVE_SEGS || npairs > 65535u)
		return -22;
	const uint32_t U     = unroll >= 4 ? 4 : 1;
	uint32_t       total = 0;
	for (uint32_t g = 0; g < T->nseg; g++) {
		tbf_move_seg&  S = T->seg[g];
		const uint64_t w = S.wide ? 16 : 8;
		if (S.bytes % w || S.srcStride % w || S.dstStride % w || (uintptr_t)S.src % w || (uintptr_t)S.dst % w)
			return -22;
		const uint64_t per = (uint64_t)SM_THREADS * U * w;
		S.slice0           = total;
		total += (uint32_t)((S.bytes + per - 1) / per);
	}
	if (total == 0)
		return 0;
	const dim3 grid (total, npairs);
	if (U == 4)
		hipLaunchKernelGGL (k_state_move<4>, grid, dim3 (SM_THREADS), 0, stream, *T, dPairSrc, dPairDst);
	else
		hipLaunchKernelGGL (k_state_move<1>, grid, dim3 (SM_THREADS), 0, stream, *T, dPairSrc, dPairDst);
	return hipGetLastError () == hipSuccess ? 0 : -5;
}
