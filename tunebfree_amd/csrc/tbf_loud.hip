/*
 * tbf_loud.hip -- k_loud, the K-weighting and hop energies of the loudness meter behind any two
 * float32 planes (tbf_loudness_device, csrc/tbf_loud.cpp): per row and channel two biquads in
 * double and the sum of squares over hops of Hp = rate / 10 frames.
 *
 * The arithmetic is include/tbf.h's definition through loud_step of csrc/tbf_loud.h, which the
 * host restatement runs too.  A channel's frames are one serial chain of dependent double
 * operations, so the kernel parallelises over rows and channels and never over a row's time: no
 * block-wise transition matrices, no tree sums, no atomics.
 *
 * A workgroup is one wave and owns TBF_LOUD_ROWS = 32 consecutive rows: lane l walks row l % 32,
 * channel l / 32, with the channel's state (five doubles, k, the hop index) in registers between
 * one load at entry and one store at exit.  Lanes of a wave read different rows, so the wave stages
 * a tile of TBF_LOUD_TILE = 128 frames of its 32 rows and 2 channels into LDS with coalesced loads
 * (64 lanes on 64 consecutive frames of one row: 256 B an instruction) and every lane walks its own
 * row of the tile from LDS, one ds_read_b128 for four frames, issued one group ahead of its use.
 * The next tile's global loads are issued into registers before the walk and are in flight during
 * it; they go to LDS when the walk is done.
 *   LDS: tile[channel][row][TBF_LOUD_PITCH] floats, the channels TBF_LOUD_PLANE floats apart.
 * PITCH = TILE + 4 puts row r's 16-byte read at banks 4 r mod 64 and
 * PLANE adds 32 for the second channel, so the four 16-lane groups of a ds_read_b128
 * ({0-3, 12-15, 20-27}, ...) each cover the 64 banks once.  The staging stores are 64 consecutive
 * dwords.
 *   Rows of a call stand at different k and take different counts, so the hop test is per lane.  A
 * group of four frames that every lane of the wave takes whole or not at all, and in which no lane
 * completes a hop, runs without tests; any other group runs the same steps with the tests per
 * frame.  A hop's energy is one ordinary global store, once per Hp frames.
 *
 * Bounds.  Global reads: in[ch][row * inStride + f] with row < nRows and f < counts[row] <= frames
 * <= inStride (checked by the host).  State: state[row * 2 + ch], row < nRows.  Energy:
 * energy[(row * maxHops + hop) * 2 + ch] with hop < maxHops (the host refuses a call that would
 * complete more, and the store tests it again).  LDS: ch * PLANE + row * PITCH + f with ch < 2,
 * row < 32; staging writes f < TILE, the walk's read-ahead reaches f < TILE + 4 behind a tile's last
 * group, which is the row's pad (PITCH = TILE + 4); what it reads there is never used.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbf_loud.h"

#define LOUD_LOADS (2u * TBF_LOUD_ROWS * (TBF_LOUD_TILE / TBF_LOUD_LANES)) /* dwords a lane loads per tile */

/* The tile from frame t0 into registers: load j is row-channel j / 2 (channel (j / 2) / 32), frame
 * t0 + 64 (j % 2) + lane.  `mine` holds row r's count in lane r, so every count is a uniform value
 * read from that lane.  A frame at or beyond its row's count is not read: the load goes to the
 * counts' own first word instead, so that all loads are issued back to back without branches. */
__device__ __forceinline__ void loud_fetch (const tbf_loud_launch& P, uint32_t mine, uint32_t row0, uint32_t t0, uint32_t lane,
                                            float (&v)[LOUD_LOADS])
{
	const float* const idle = reinterpret_cast<const float*> (P.counts);
#pragma unroll
	for (uint32_t j = 0; j < LOUD_LOADS; j++) {
		const uint32_t rc = j / 2u, r = rc % TBF_LOUD_ROWS, ch = rc / TBF_LOUD_ROWS;
		const uint32_t f = t0 + (j % 2u) * TBF_LOUD_LANES + lane;
		const uint32_t c = (uint32_t)__builtin_amdgcn_readlane ((int)mine, (int)r);
		const float*   p = P.in[ch] + (uint64_t)(row0 + r) * P.inStride + f;
		v[j]             = *(f < c ? p : idle);
	}
}

__global__ __launch_bounds__ (TBF_LOUD_LANES) void k_loud (tbf_loud_launch P)
{
	__shared__ float4 lds4[TBF_LOUD_LDS_BYTES / 16u];
	float* const      tile = reinterpret_cast<float*> (lds4);

	const uint32_t lane = threadIdx.x, r = lane % TBF_LOUD_ROWS, ch = lane / TBF_LOUD_ROWS;
	const uint32_t row0 = blockIdx.x * TBF_LOUD_ROWS, row = row0 + r;

	/* the counts of the workgroup's rows (0 beyond the meter's last), and the largest */
	const uint32_t mine = row < P.nRows ? P.counts[row] : 0u;
	uint32_t       most = mine;
#pragma unroll
	for (int d = 16; d; d >>= 1)
		most = max (most, (uint32_t)__shfl_xor ((int)most, d));
	if (most == 0)
		return;

	tbf_loud_chan S = {0.0, 0.0, 0.0, 0.0, 0.0, 0u, 0u};
	if (mine)
		S = P.state[(uint64_t)row * 2u + ch];
	const uint32_t Hp      = P.Hp;
	double* const  erow    = P.energy + (uint64_t)row * P.maxHops * 2u + ch;
	const float*   my      = tile + ch * TBF_LOUD_PLANE + r * TBF_LOUD_PITCH;
	const double   c[7]    = {P.c[0], P.c[1], P.c[2], P.c[3], P.c[4], P.c[5], P.c[6]};

	float v[LOUD_LOADS];
	loud_fetch (P, mine, row0, 0u, lane, v);
	for (uint32_t t0 = 0; t0 < most; t0 += TBF_LOUD_TILE) {
		/* the fetched tile to LDS */
#pragma unroll
		for (uint32_t j = 0; j < LOUD_LOADS; j++) {
			const uint32_t rc = j / 2u;
			tile[(rc / TBF_LOUD_ROWS) * TBF_LOUD_PLANE + (rc % TBF_LOUD_ROWS) * TBF_LOUD_PITCH + (j % 2u) * TBF_LOUD_LANES + lane] = v[j];
		}
		__syncthreads ();
		if (t0 + TBF_LOUD_TILE < most) /* the next one's loads, in flight during the walk */
			loud_fetch (P, mine, row0, t0 + TBF_LOUD_TILE, lane, v);

		/* the walk: n frames of this tile are the lane's, the wave goes to the largest n */
		const uint32_t n    = mine > t0 ? min (mine - t0, TBF_LOUD_TILE) : 0u;
		const uint32_t nMax = min (most - t0, TBF_LOUD_TILE);
		float4         nx   = *reinterpret_cast<const float4*> (my);
		for (uint32_t f = 0; f < nMax; f += TBF_LOUD_GROUP) {
			const float4 q = nx;
			nx             = *reinterpret_cast<const float4*> (my + f + TBF_LOUD_GROUP); /* the pad holds the last one */
			const float x[TBF_LOUD_GROUP] = {q.x, q.y, q.z, q.w};
			if (__all (f >= n || (f + TBF_LOUD_GROUP <= n && S.k + TBF_LOUD_GROUP < Hp))) {
				if (f < n) {
#pragma unroll
					for (uint32_t i = 0; i < TBF_LOUD_GROUP; i++)
						loud_step (c, (double)x[i], S);
				}
			} else {
#pragma unroll
				for (uint32_t i = 0; i < TBF_LOUD_GROUP; i++)
					if (f + i < n) {
						loud_step (c, (double)x[i], S);
						if (S.k == Hp) {
							if (S.hop < P.maxHops)
								erow[(uint64_t)S.hop * 2u] = S.acc;
							S.acc = 0.0;
							S.k   = 0u;
							S.hop = S.hop + 1u;
						}
					}
			}
		}
		__syncthreads ();
	}
	if (mine)
		P.state[(uint64_t)row * 2u + ch] = S;
}

extern "C" int tbf_launch_loud (const tbf_loud_launch* P, hipStream_t stream)
{
	if (P->nRows == 0)
		return 0;
	if (!P->in[0] || !P->in[1] || !P->counts || !P->state || !P->energy || P->Hp == 0)
		return -5;
	hipLaunchKernelGGL (k_loud, dim3 ((P->nRows + TBF_LOUD_ROWS - 1u) / TBF_LOUD_ROWS), dim3 (TBF_LOUD_LANES), 0, stream, *P);
	return hipGetLastError () == hipSuccess ? 0 : -5;
}
