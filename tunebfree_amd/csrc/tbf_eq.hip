/*
 * tbf_eq.hip -- k_eq, the bus equaliser behind any two float32 planes (tbf_eq_device,
 * csrc/tbf_eq.cpp): per row and channel a cascade of up to eight biquads in double, transposed
 * direct form II, the bands of one row-channel as a systolic pipeline across adjacent lanes.
 *
 * The arithmetic is include/tbf.h's definition through eq_step of csrc/tbf_eq.h, which the host
 * restatement runs too.  A band's frames are one serial chain of dependent double operations, and
 * band b of frame n needs only band b - 1 of frame n and its own state of frame n - 1.  So the
 * kernel parallelises over rows, channels and bands, never over a row's time: no transition
 * matrices, no tree sums, no atomics, and every operation and its order are the serial cascade's.
 *
 * A workgroup is one wave.  P = eq_lanes (maxBands) adjacent lanes serve one row-channel: lane l is
 * band b = l % P of row-channel g = l / P, which is row g % (32 / P), channel g / (32 / P) of the
 * wave's 32 / P consecutive rows.  P divides 16, so a row-channel never leaves a DPP row.  A lane
 * holds its band's five coefficients and two state doubles in registers from one load at entry to
 * one store at exit; a lane whose band the row does not use (b >= nb[row]) loads and stores nothing.
 *   The pipeline.  At step t of a tile lane b takes frame t - b: band 0 from the staged input, band
 * b > 0 from what lane b - 1 put out the step before, which reaches it as two 32-bit DPP moves
 * (row_shr:1); the lane at a row-channel's start ignores what is shifted in.  A lane without a band
 * hands its input on by a select, so lane P - 1 always holds the row-channel's output, which it
 * writes over the frame's input in the tile.  A tile of n frames runs n + P - 1 steps and ends
 * drained: nothing in flight crosses a tile, let alone a call, and the P - 1 idle steps per tile of
 * TBF_EQ_TILE = 128 frames cost at most 7 / 135 of the steps (P = 8).  The other choice, an output
 * tile that lags the input tile by P - 1 frames, saves those steps and needs a second tile in LDS
 * and stores that straddle two tiles; it was not taken.
 *   Staging as k_loud's: the wave loads a tile of its row-channels with coalesced loads (64 lanes on
 * 64 consecutive frames of one row: 256 B an instruction), the next tile's loads are issued into
 * registers before the walk and are in flight during it.  A lane reads its row-channel's next four
 * frames with one ds_read_b128, one group ahead of their use (the P lanes of a row-channel read one
 * address; only band 0 uses it).  When the walk is done the tile, now the output, goes to global
 * memory with coalesced stores.
 *   LDS: tile[row-channel g] at eq_lds_off (g) = g * TBF_EQ_PITCH + 32 (g / 32) floats.  PITCH =
 * TILE + 4 puts row-channel g's 16-byte read at banks 4 g mod 64 and the second 32 row-channels
 * (P = 1 only) half a bank row further, as k_loud's planes.  Lane P - 1's write of frame t - (P - 1)
 * goes to bank 4 g + t - (P - 1), behind band 0's read of frames t + 4 .. t + 7 of the same step
 * group, and is a single dword off the recurrence's critical path.
 *   Rows of a call take different counts and the lanes of a row-channel stand at different frames,
 * so whether a lane's step counts is per lane.  A group of four steps in which every lane of the
 * wave either takes four frames or is past its row's last runs without tests (the lanes of one
 * row-channel are then all of one kind, so the DPP moves stay inside enabled lanes); any other
 * group, a tile's first and last ones, runs the same steps with the test per step and the state
 * kept by selects.
 *
 * Bounds.  Global reads: in[ch][row * inStride + f] with row < nRows and f < count (row) <= frames
 * <= inStride (checked by the host); a frame at or beyond the count reads nb[0] instead.  Global
 * writes: out[ch][row * outStride + f], the same limits with outStride.  nb[row], coef[(row *
 * maxBands + b) * 5 + 0..4] and state[((row * 2 + ch) * maxBands + b) * 2 + 0..1] with row < nRows,
 * ch < 2 and b < nb[row] <= maxBands (the host's tables hold nothing else).  LDS: eq_lds_off (g) + f
 * with g < 64 / P; staging writes and the output reads f < TILE; the walk reads f < TILE + 4 (the
 * read-ahead stops at the row-channel's pad, PITCH = TILE + 4; what it reads there is never used)
 * and writes frames f < n <= TILE; the last row-channel ends at eq_lds_floats (P).
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbf_eq.h"

/* x of the lane one below, within a DPP row of 16 lanes; a row's first lane keeps its own */
__device__ __forceinline__ double eq_from_below (double x)
{
	int lo = __double2loint (x), hi = __double2hiint (x);
	lo     = __builtin_amdgcn_update_dpp (lo, lo, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
	hi     = __builtin_amdgcn_update_dpp (hi, hi, 0x111, 0xf, 0xf, false);
	return __hiloint2double (hi, lo);
}

/* one step of a lane: its input from the tile (band 0) or from the lane below, through its band
 * when it holds one (`on`), else handed on; the state moves when the step counts */
template <uint32_t P, bool TEST>
__device__ __forceinline__ void eq_lane_step (const double* c, bool on, bool head, bool act, float x, double& y, double& s1, double& s2)
{
	/* the move before the select, by every lane: a DPP move reads nothing from a lane that is
	 * switched off, and inside `head ? .. : ..` the heads would be */
	const double below = P == 1u ? 0.0 : eq_from_below (y);
	const double v     = (P == 1u || head) ? (double)x : below;
	double       t1 = s1, t2 = s2;
	const double w  = eq_step (c, v, t1, t2);
	y               = on ? w : v;
	if (!TEST || (act && on)) {
		s1 = t1;
		s2 = t2;
	}
}

/* The tile from frame t0 into registers: load j is row-channel j / 2, frame t0 + 64 (j % 2) + lane.
 * `mine` holds row r's count in lane r * P, so every count is a uniform value read from that lane.
 * A frame at or beyond its row's count is not read: the load goes to the band counts' first word
 * instead, so that all loads are issued back to back without branches. */
template <uint32_t P>
__device__ __forceinline__ void eq_fetch (const tbf_eq_launch& A, uint32_t mine, uint32_t row0, uint32_t t0, uint32_t lane,
                                          float (&v)[(64u / P) * (TBF_EQ_TILE / TBF_EQ_LANES)])
{
	constexpr uint32_t RW = 32u / P, PER = TBF_EQ_TILE / TBF_EQ_LANES;
	const float* const idle = reinterpret_cast<const float*> (A.nb);
#pragma unroll
	for (uint32_t j = 0; j < (64u / P) * PER; j++) {
		const uint32_t rc = j / PER, r = rc % RW, ch = rc / RW;
		const uint32_t f  = t0 + (j % PER) * TBF_EQ_LANES + lane;
		const uint32_t n  = (uint32_t)__builtin_amdgcn_readlane ((int)mine, (int)(r * P));
		const float*   p  = A.in[ch] + (uint64_t)(row0 + r) * A.inStride + f;
		v[j]              = *(f < n ? p : idle);
	}
}

template <uint32_t P>
__global__ __launch_bounds__ (TBF_EQ_LANES) void k_eq (tbf_eq_launch A)
{
	constexpr uint32_t RC = 64u / P, RW = 32u / P, PER = TBF_EQ_TILE / TBF_EQ_LANES, LOADS = RC * PER;
	__shared__ float4  lds4[(eq_lds_floats (P) + 3u) / 4u];
	float* const       tile = reinterpret_cast<float*> (lds4);

	const uint32_t lane = threadIdx.x, b = lane % P, g = lane / P, r = g % RW, ch = g / RW;
	const uint32_t row0 = blockIdx.x * RW, row = row0 + r;

	/* the counts of the wave's rows (0 beyond the equaliser's last), and the largest */
	const uint32_t mine = row < A.nRows ? (A.counts ? A.counts[row] : A.frames) : 0u;
	uint32_t       most = mine;
#pragma unroll
	for (int d = 32; d; d >>= 1)
		most = max (most, (uint32_t)__shfl_xor ((int)most, d));
	if (most == 0)
		return;

	const bool    on = mine && b < A.nb[row]; /* the lane holds a band of a row that takes frames */
	const bool    head = b == 0u, tail = b == P - 1u;
	double        c[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, s1 = 0.0, s2 = 0.0;
	double* const st   = A.state + (((uint64_t)row * 2u + ch) * A.maxBands + b) * 2u;
	if (on) {
		const double* const cr = A.coef + ((uint64_t)row * A.maxBands + b) * 5u;
#pragma unroll
		for (int i = 0; i < 5; i++)
			c[i] = cr[i];
		s1 = st[0];
		s2 = st[1];
	}
	float* const my = tile + eq_lds_off (g);

	float v[LOADS];
	eq_fetch<P> (A, mine, row0, 0u, lane, v);
	for (uint32_t t0 = 0; t0 < most; t0 += TBF_EQ_TILE) {
		/* the fetched tile to LDS */
#pragma unroll
		for (uint32_t j = 0; j < LOADS; j++)
			tile[eq_lds_off (j / PER) + (j % PER) * TBF_EQ_LANES + lane] = v[j];
		__syncthreads ();
		if (t0 + TBF_EQ_TILE < most) /* the next one's loads, in flight during the walk */
			eq_fetch<P> (A, mine, row0, t0 + TBF_EQ_TILE, lane, v);

		/* the walk: n frames of this tile are the lane's row's, the wave goes to the largest n and
		 * P - 1 steps beyond, which drain the pipeline */
		const int      n     = (int)(mine > t0 ? min (mine - t0, TBF_EQ_TILE) : 0u);
		const uint32_t steps = min (most - t0, TBF_EQ_TILE) + P - 1u;
		double         y     = 0.0;
		float4         nx    = *reinterpret_cast<const float4*> (my);
		for (uint32_t t = 0; t < steps; t += TBF_EQ_GROUP) {
			const float4 q = nx;
			nx             = *reinterpret_cast<const float4*> (my + min (t + TBF_EQ_GROUP, TBF_EQ_TILE)); /* the pad holds the last one */
			const float x[TBF_EQ_GROUP] = {q.x, q.y, q.z, q.w};
			const int   f0   = (int)t - (int)b; /* the lane's frame at the group's first step */
			const bool  past = f0 >= n, whole = f0 >= 0 && f0 + (int)TBF_EQ_GROUP <= n;
			if (__all (past || whole)) {
				if (whole) {
					float o[TBF_EQ_GROUP];
#pragma unroll
					for (uint32_t i = 0; i < TBF_EQ_GROUP; i++) {
						eq_lane_step<P, false> (c, on, head, true, x[i], y, s1, s2);
						o[i] = (float)y;
					}
					if (tail) {
#pragma unroll
						for (uint32_t i = 0; i < TBF_EQ_GROUP; i++)
							my[f0 + (int)i] = o[i];
					}
				}
			} else {
#pragma unroll
				for (uint32_t i = 0; i < TBF_EQ_GROUP; i++) {
					const int  f   = f0 + (int)i;
					const bool act = f >= 0 && f < n;
					eq_lane_step<P, true> (c, on, head, act, x[i], y, s1, s2);
					if (tail && act)
						my[f] = (float)y;
				}
			}
		}
		__syncthreads ();
		/* the tile, now the output, to global memory */
#pragma unroll
		for (uint32_t j = 0; j < LOADS; j++) {
			const uint32_t rc = j / PER, rr = rc % RW, cc = rc / RW;
			const uint32_t f  = t0 + (j % PER) * TBF_EQ_LANES + lane;
			const uint32_t nn = (uint32_t)__builtin_amdgcn_readlane ((int)mine, (int)(rr * P));
			if (f < nn)
				A.out[cc][(uint64_t)(row0 + rr) * A.outStride + f] = tile[eq_lds_off (rc) + (j % PER) * TBF_EQ_LANES + lane];
		}
		__syncthreads ();
	}
	if (on) {
		st[0] = s1;
		st[1] = s2;
	}
}

extern "C" int tbf_launch_eq (const tbf_eq_launch* A, hipStream_t stream)
{
	if (A->nRows == 0 || A->frames == 0)
		return 0;
	if (!A->in[0] || !A->in[1] || !A->out[0] || !A->out[1] || !A->nb || !A->coef || !A->state || A->maxBands < 1u || A->maxBands > 8u)
		return -5;
	const uint32_t P = eq_lanes (A->maxBands), RW = eq_rows (P);
	const dim3     grid ((A->nRows + RW - 1u) / RW), block (TBF_EQ_LANES);
	switch (P) {
		case 1: hipLaunchKernelGGL (k_eq<1u>, grid, block, 0, stream, *A); break;
		case 2: hipLaunchKernelGGL (k_eq<2u>, grid, block, 0, stream, *A); break;
		case 4: hipLaunchKernelGGL (k_eq<4u>, grid, block, 0, stream, *A); break;
		default: hipLaunchKernelGGL (k_eq<8u>, grid, block, 0, stream, *A); break;
	}
	return hipGetLastError () == hipSuccess ? 0 : -5;
}
