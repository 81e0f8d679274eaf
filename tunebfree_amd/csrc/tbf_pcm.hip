/*
 * tbf_pcm.hip -- k_pcm, the PCM output stage behind L / R (tbf_pcm_convert_device and the
 * tbf_render_pcm* / tbf_process_pcm* calls, csrc/tbf_pcm.cpp): two float32 planes into interleaved
 * int16 / packed int24 / float32 frames, with a peak and a clip count per row and channel.
 *
 * The arithmetic is include/tbf.h's definition, through the functions of csrc/tbf_pcm.h that the
 * host restatement runs too.  It is per sample and the dither is a function of (seed, row,
 * channel, frame), so a row's bytes are the same however a call is cut.
 *
 * Pure streaming: 8 B in and 4 / 6 / 8 B out per frame.  The grid is (tile, row); a workgroup of
 * TBF_PCM_LANES lanes owns TBF_PCM_TILE consecutive frames of one row and a lane
 * TBF_PCM_GROUP = 4 consecutive ones, so a full lane reads 16 B of each plane and writes 16 / 24 /
 * 32 B, neighbouring lanes next to each other.  Rows have their own counts: a tile beyond its
 * row's count exits.
 * Loads: one dwordx4 per plane when both of the row's input addresses are 16-byte aligned (the
 * tbf_render_device contract allows any float alignment and odd strides, so this is decided per
 * row), four dwords otherwise, and in the lane that holds the row's last, partial group.
 * Stores: whole dwords.  When the row's output address is 16-byte aligned a full lane stores one
 * dwordx4 (S16), three dwordx2 (S24: 24 B per lane keep 8-byte alignment) or two dwordx4 (F32);
 * otherwise, and in the last partial group, dword by dword.  Only an S24 row with an odd count
 * ends in a 2-byte store.  Nothing outside [0, count * frame bytes) of a row is written.
 * Meters: each lane's peak (as the bits of a non-negative float, which order as the floats do)
 * and clip counts are reduced over the wave with shuffles, then one integer atomicMax and one
 * integer atomicAdd per wave and channel, skipped when they would add nothing.  Integer maxima
 * and sums do not depend on order, so the meters are exact however the grid is scheduled and
 * however a call is cut.  The caller zeroes the meters once per call.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbf_pcm.h"

template <int FMT, bool DITHER>
__global__ __launch_bounds__ (TBF_PCM_LANES) void k_pcm (tbf_pcm_launch P)
{
	const uint32_t row   = P.rowBase + blockIdx.y, lane = threadIdx.x;
	const uint32_t count = P.rowCounts ? P.rows[row].count : P.countU;
	const uint64_t t0    = (uint64_t)blockIdx.x * TBF_PCM_TILE;
	if (t0 >= count)
		return;
	const uint64_t j  = t0 + (uint64_t)lane * TBF_PCM_GROUP; /* the lane's first frame */
	const uint32_t nf = j < count ? (uint32_t)min ((uint64_t)TBF_PCM_GROUP, count - j) : 0u;
	const uint32_t* __restrict__ inL = reinterpret_cast<const uint32_t*> (P.in[0] + (uint64_t)row * P.inStride);
	const uint32_t* __restrict__ inR = reinterpret_cast<const uint32_t*> (P.in[1] + (uint64_t)row * P.inStride);
	unsigned char* const out         = P.out + (uint64_t)row * P.outStride;
	const bool           inWide      = (((uintptr_t)inL | (uintptr_t)inR) & 15u) == 0;
	const bool           outWide     = ((uintptr_t)out & 15u) == 0;
	constexpr uint32_t   FB          = FMT == TBF_PCM_S16 ? 4u : FMT == TBF_PCM_S24_3LE ? 6u : 8u;

	uint32_t l[4] = {0u, 0u, 0u, 0u}, r[4] = {0u, 0u, 0u, 0u};
	if (nf == TBF_PCM_GROUP && inWide) {
		const uint4 a = *reinterpret_cast<const uint4*> (inL + j), b = *reinterpret_cast<const uint4*> (inR + j);
		l[0] = a.x, l[1] = a.y, l[2] = a.z, l[3] = a.w;
		r[0] = b.x, r[1] = b.y, r[2] = b.z, r[3] = b.w;
	} else {
#pragma unroll
		for (uint32_t k = 0; k < TBF_PCM_GROUP; k++)
			if (k < nf) {
				l[k] = inL[j + k];
				r[k] = inR[j + k];
			}
	}

	pcm_acc  m = {{0u, 0u}, {0u, 0u}};
	uint32_t w[8];
	uint32_t bytes = 0;
	if (nf) {
		const uint64_t f = (P.rows ? P.rows[row].frame0 : P.frame0U) + P.frameOff + j;
		bytes            = pcm_group<FMT, DITHER> (l, r, nf, P.seed, row, f, w, m);
	}

	if (nf) {
		unsigned char* const o = out + j * FB; /* a multiple of 4 FB bytes into the row */
		if (nf == TBF_PCM_GROUP && outWide) {
			if (FMT == TBF_PCM_S16) {
				*reinterpret_cast<uint4*> (o) = make_uint4 (w[0], w[1], w[2], w[3]);
			} else if (FMT == TBF_PCM_S24_3LE) {
				uint2* const o2 = reinterpret_cast<uint2*> (o);
				o2[0]           = make_uint2 (w[0], w[1]);
				o2[1]           = make_uint2 (w[2], w[3]);
				o2[2]           = make_uint2 (w[4], w[5]);
			} else {
				uint4* const o4 = reinterpret_cast<uint4*> (o);
				o4[0]           = make_uint4 (w[0], w[1], w[2], w[3]);
				o4[1]           = make_uint4 (w[4], w[5], w[6], w[7]);
			}
		} else {
			uint32_t* const o1 = reinterpret_cast<uint32_t*> (o);
#pragma unroll
			for (uint32_t k = 0; k < 8; k++)
				if (4 * k + 4 <= bytes)
					o1[k] = w[k];
			if (FMT == TBF_PCM_S24_3LE && (bytes & 2u)) /* nf 1 or 3: 6 or 18 bytes */
				*reinterpret_cast<uint16_t*> (o + (bytes & ~3u)) = (uint16_t)(nf == 1 ? w[1] : w[4]);
		}
	}

	if (P.meters) { /* uniform over the launch: every lane of the wave takes part, idle ones with zeros */
#pragma unroll
		for (int d = 32; d; d >>= 1) {
			m.peak[0] = max (m.peak[0], (uint32_t)__shfl_xor ((int)m.peak[0], d));
			m.peak[1] = max (m.peak[1], (uint32_t)__shfl_xor ((int)m.peak[1], d));
			m.clip[0] += (uint32_t)__shfl_xor ((int)m.clip[0], d);
			m.clip[1] += (uint32_t)__shfl_xor ((int)m.clip[1], d);
		}
		if ((lane & 63u) == 0) {
			tbf_pcm_meter* const t = P.meters + row;
			if (m.peak[0])
				atomicMax (reinterpret_cast<unsigned int*> (&t->peakL), m.peak[0]);
			if (m.peak[1])
				atomicMax (reinterpret_cast<unsigned int*> (&t->peakR), m.peak[1]);
			if (m.clip[0])
				atomicAdd (&t->clipL, m.clip[0]);
			if (m.clip[1])
				atomicAdd (&t->clipR, m.clip[1]);
		}
	}
}

template <int FMT, bool DITHER>
static int pcm_launch (const tbf_pcm_launch& P, hipStream_t stream)
{
	const uint32_t tiles = (uint32_t)(((uint64_t)P.maxCount + TBF_PCM_TILE - 1) / TBF_PCM_TILE);
	hipLaunchKernelGGL ((k_pcm<FMT, DITHER>), dim3 (tiles, P.nRows), dim3 (TBF_PCM_LANES), 0, stream, P);
	return hipGetLastError () == hipSuccess ? 0 : -5;
}

extern "C" int tbf_launch_pcm (const tbf_pcm_launch* P, hipStream_t stream)
{
	if (P->nRows == 0 || P->maxCount == 0)
		return 0;
	if (P->nRows > TBF_PCM_MAX_ROWS || (P->rowCounts && !P->rows))
		return -5;
	switch (P->format) {
	case TBF_PCM_S16:
		return (P->flags & TBF_PCM_DITHER) ? pcm_launch<TBF_PCM_S16, true> (*P, stream) : pcm_launch<TBF_PCM_S16, false> (*P, stream);
	case TBF_PCM_S24_3LE:
		return pcm_launch<TBF_PCM_S24_3LE, false> (*P, stream);
	case TBF_PCM_F32:
		return pcm_launch<TBF_PCM_F32, false> (*P, stream);
	}
	return -5;
}
