/*
 * tbf_cabinet.hip -- k_cabinet, the cabinet convolver behind the rotor planes
 * (tbf_render_cabinet* / tbf_process_cabinet*, csrc/tbf_cabinet.cpp).
 *
 * Per instance and channel: wet = horn * ir (hornL with irL, hornR with irR, no cross terms),
 * then out = (dry * horn + wet_mix * wet) + drum, every operation of that line one float32
 * operation.  The convolution is uniformly partitioned overlap-save at the block size
 * (csrc/tbf_cabinet.h): X_b = FFT-256 of blocks (b - 1, b), Y_b = sum over k = 0 .. K - 1 of
 * X_{b-k} H_k in ascending k (all K terms always, zero spectra before an instance's first
 * block), block b of wet = the last 128 points of IFFT-256 (Y_b).  Every block takes the same
 * instructions whatever the call or chunk it arrives in, so the planes are bit-identical at
 * every cut.
 *
 * One wave64 workgroup per (instance, channel) walks the call's blocks in order, TBF_CAB_TILE
 * at a time.  Lane l owns the packed bins l and l + 64 of every spectrum of its row, in the
 * ring, in the registers and in H: what a lane reads from the ring it wrote itself.
 *   pass 1  the tile's blocks: FFT, spectrum into its ring slot
 *   pass 2  k = 0 .. K - 1: one load of H_k's two bins serves the tile's (up to) 8 output
 *           blocks; the spectra X_{b-k} slide through a register window, one ring load per k
 *   pass 3  the tile's blocks: IFFT, mix, store
 * So H (K KB per channel, shared by every row) and the ring are each read once per tile, not
 * once per block, and a tile's horn and drum samples come in one round of loads each.  The FFT is
 * radix-2 on the full complex frame (forward: decimation in frequency, natural in, bit-reversed
 * out; inverse: decimation in time, bit-reversed in, natural out): the two widest stages in the
 * lane's own registers (a lane holds points l, l + 64, l + 128, l + 192), the six others in LDS
 * (separate re and im arrays: interleaved pairs measured 3 to 7 % slower);
 * twiddles from a table built on the host in double.
 * Memory per instance: 2 x (16 + 512 + (K + 7) x 1024) bytes of state; no per-sample scratch of
 * its own (the rotor planes it reads are the caller's or the engine's, csrc/tbf_cabinet.cpp).
 * Rows are read and written one float at a time inside [0, nb * 128) only.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tbf_cabinet.h"

#define CB_T TBF_CAB_TILE

/* position of bin j in a bit-reversed 256-point frame */
__device__ __forceinline__ uint32_t cb_rev (uint32_t j) { return __brev (j) >> 24; }

/* the two butterflies every stage is made of, the same instructions wherever a stage runs.
 * dif: (u + v, (u - v) w); dit with the conjugate twiddle: (u + v w*, u - v w*); w = (wr, wi) is
 * the table's exp (-2 pi i t / 256) */
__device__ __forceinline__ void cb_dif (float& ar, float& ai, float& br, float& bi, float wr, float wi)
{
	const float dr = ar - br, di = ai - bi;
	ar = ar + br;
	ai = ai + bi;
	br = dr * wr - di * wi;
	bi = dr * wi + di * wr;
}

__device__ __forceinline__ void cb_dit (float& ar, float& ai, float& br, float& bi, float wr, float wi)
{
	const float xr = br * wr + bi * wi, xi = bi * wr - br * wi; /* v times the conjugate of w */
	br = ar - xr;
	bi = ai - xi;
	ar = ar + xr;
	ai = ai + xi;
}

/* one radix-2 stage over the 256-point frame in LDS: 128 butterflies, two a lane; m: the
 * butterfly's half span, shift: log2 (128 / m) */
template <bool DIF>
__device__ __forceinline__ void cb_stage (float* re, float* im, const float* twc, const float* tws, uint32_t m,
                                          uint32_t shift)
{
#pragma unroll
	for (uint32_t q = 0; q < 2; q++) {
		const uint32_t i = threadIdx.x + 64 * q;
		const uint32_t p = i & (m - 1);
		const uint32_t a = ((i - p) << 1) + p, b = a + m;
		const uint32_t t = p << shift; /* p * (128 / m) */
		float          ar = re[a], ai = im[a], br = re[b], bi = im[b];
		if (DIF)
			cb_dif (ar, ai, br, bi, twc[t], tws[t]);
		else
			cb_dit (ar, ai, br, bi, twc[t], tws[t]);
		re[a] = ar;
		im[a] = ai;
		re[b] = br;
		im[b] = bi;
	}
	__syncthreads ();
}

/* a lane's twiddles for the two stages it runs in its own registers (spans 128 and 64: lane l
 * holds points l, l + 64, l + 128, l + 192, which those stages pair among themselves) */
struct cb_tw {
	float c0, s0, c1, s1, c2, s2; /* t = l, l + 64 (span 128), 2 l (span 64) */
};

/* forward: the real frame x[0..3] = points l, l + 64, l + 128, l + 192 -> bit-reversed spectrum in LDS */
__device__ __forceinline__ void cb_fft (const float x[4], float* re, float* im, const float* twc, const float* tws,
                                        const cb_tw& W)
{
	const uint32_t l = threadIdx.x;
	float r0 = x[0], r1 = x[1], r2 = x[2], r3 = x[3], i0 = 0.0f, i1 = 0.0f, i2 = 0.0f, i3 = 0.0f;
	cb_dif (r0, i0, r2, i2, W.c0, W.s0); /* span 128 */
	cb_dif (r1, i1, r3, i3, W.c1, W.s1);
	cb_dif (r0, i0, r1, i1, W.c2, W.s2); /* span 64 */
	cb_dif (r2, i2, r3, i3, W.c2, W.s2);
	re[l]       = r0;
	im[l]       = i0;
	re[l + 64]  = r1;
	im[l + 64]  = i1;
	re[l + 128] = r2;
	im[l + 128] = i2;
	re[l + 192] = r3;
	im[l + 192] = i3;
	__syncthreads ();
	uint32_t shift = 2;
	for (uint32_t m = 32; m >= 1; m >>= 1, shift++)
		cb_stage<true> (re, im, twc, tws, m, shift);
}

/* inverse: bit-reversed spectrum in LDS -> the real parts of points l + 128 and l + 192 (times 256) */
__device__ __forceinline__ void cb_ifft (float* re, float* im, const float* twc, const float* tws, const cb_tw& W,
                                         float& y0, float& y1)
{
	const uint32_t l = threadIdx.x;
	uint32_t       shift = 7;
	for (uint32_t m = 1; m <= 32; m <<= 1, shift--)
		cb_stage<false> (re, im, twc, tws, m, shift);
	float r0 = re[l], r1 = re[l + 64], r2 = re[l + 128], r3 = re[l + 192];
	float i0 = im[l], i1 = im[l + 64], i2 = im[l + 128], i3 = im[l + 192];
	cb_dit (r0, i0, r1, i1, W.c2, W.s2); /* span 64 */
	cb_dit (r2, i2, r3, i3, W.c2, W.s2);
	cb_dit (r0, i0, r2, i2, W.c0, W.s0); /* span 128 */
	cb_dit (r1, i1, r3, i3, W.c1, W.s1);
	y0 = r2;
	y1 = r3;
}

__global__ __launch_bounds__ (64, 2) void k_cabinet (tbf_cab_launch P)
{
	__shared__ float re[TBF_CAB_FFT], im[TBF_CAB_FFT], twc[128], tws[128];
	const uint32_t l = threadIdx.x, inst = blockIdx.x >> 1, ch = blockIdx.x & 1;
	const uint32_t K = P.K, R = P.R, nb = P.nb;
	twc[l]      = P.tw[l];
	twc[l + 64] = P.tw[l + 64];
	tws[l]      = P.tw[128 + l];
	tws[l + 64] = P.tw[128 + l + 64];
	const cb_tw W = {P.tw[l], P.tw[128 + l], P.tw[l + 64], P.tw[128 + l + 64], P.tw[(2 * l) & 127], P.tw[128 + ((2 * l) & 127)]};
	float* const    S    = P.state + ((uint64_t)inst * 2 + ch) * P.chFloats;
	const uint32_t  pos  = *reinterpret_cast<const uint32_t*> (S); /* ring slot of the call's first block */
	float* const    tail = S + TBF_CAB_HDR;
	float2* const   ring = reinterpret_cast<float2*> (S + TBF_CAB_HDR + TBF_CAB_PART);
	const float2*   H    = reinterpret_cast<const float2*> (P.H[ch]);
	const float*    horn = P.horn[ch] + (uint64_t)inst * P.rotStride;
	const float*    drum = P.drum[ch] + (uint64_t)inst * P.rotStride;
	float* const    out  = P.out[ch] + (uint64_t)inst * P.outStride;
	float* const    wout = P.wet[ch] ? P.wet[ch] + (uint64_t)inst * P.outStride : nullptr;
	const bool      dc   = l == 0; /* this lane's first bin is the packed (DC, Nyquist) pair */
	const float     mix0 = P.wet0[inst];
	float           p0 = tail[l], p1 = tail[l + 64]; /* the block before the tile */
	__syncthreads ();

	for (uint32_t b0 = 0; b0 < nb; b0 += CB_T) {
		const uint32_t tn = min ((uint32_t)CB_T, nb - b0);
		/* the tile's horn samples: one round of loads for the FFTs and the mix */
		float hx[CB_T][2];
#pragma unroll
		for (int t = 0; t < CB_T; t++) {
			hx[t][0] = hx[t][1] = 0.0f;
			if ((uint32_t)t < tn) {
				const float* cur = horn + (uint64_t)(b0 + t) * TBF_CAB_PART;
				hx[t][0] = cur[l];
				hx[t][1] = cur[l + 64];
			}
		}
		/* pass 1: the spectra of the tile's blocks into the ring */
#pragma unroll
		for (int t = 0; t < CB_T; t++) {
			if ((uint32_t)t >= tn)
				break;
			const float x[4] = {t ? hx[t ? t - 1 : 0][0] : p0, t ? hx[t ? t - 1 : 0][1] : p1, hx[t][0], hx[t][1]};
			cb_fft (x, re, im, twc, tws, W);
			const uint32_t r0 = cb_rev (l), r1 = cb_rev (l + 64);
			float2         x0 = make_float2 (re[r0], im[r0]);
			if (dc)
				x0.y = re[cb_rev (128)];
			const float2   x1   = make_float2 (re[r1], im[r1]);
			float2* const  slot = ring + (uint64_t)((pos + b0 + t) % R) * 128;
			slot[l]      = x0;
			slot[l + 64] = x1;
			__syncthreads ();
		}
		/* pass 2: Y_{b0+t} = sum_k X_{b0+t-k} H_k, ascending k; w?[t] holds X_{b0+t-k}.  The loads
		 * of step k + 1 (H_{k+1}, and the spectrum that enters the window then) go out before step k's arithmetic */
		float2 w0[CB_T], w1[CB_T], a0[CB_T], a1[CB_T];
#pragma unroll
		for (int t = 0; t < CB_T; t++) {
			a0[t] = a1[t] = make_float2 (0.0f, 0.0f);
			w0[t] = w1[t] = make_float2 (0.0f, 0.0f);
			if ((uint32_t)t < tn) {
				const float2* slot = ring + (uint64_t)((pos + b0 + t) % R) * 128;
				w0[t] = slot[l];
				w1[t] = slot[l + 64];
			}
		}
		float2 nh0 = H[l], nh1 = H[64 + l], nx0 = make_float2 (0.0f, 0.0f), nx1 = nx0;
		if (K > 1) { /* X_{b0-1}: up to K - 1 < R blocks back, slots this tile has not written */
			const float2* slot = ring + (uint64_t)((pos + b0 + R - 1) % R) * 128;
			nx0 = slot[l];
			nx1 = slot[l + 64];
		}
		for (uint32_t k = 0; k < K; k++) {
			const float2 h0 = nh0, h1 = nh1, x0 = nx0, x1 = nx1;
			if (k + 1 < K) {
				nh0 = H[(uint64_t)(k + 1) * 128 + l];
				nh1 = H[(uint64_t)(k + 1) * 128 + 64 + l];
			}
			if (k + 2 < K) {
				const float2* slot = ring + (uint64_t)((pos + b0 + R - (k + 2)) % R) * 128;
				nx0 = slot[l];
				nx1 = slot[l + 64];
			}
			/* the packed pair multiplies component by component, every other bin as a complex number */
			const float c0 = h0.x, c1 = dc ? 0.0f : h0.y, c2 = dc ? h0.y : h0.x;
#pragma unroll
			for (int t = 0; t < CB_T; t++) {
				a0[t].x = fmaf (w0[t].x, c0, a0[t].x);
				a0[t].x = fmaf (-w0[t].y, c1, a0[t].x);
				a0[t].y = fmaf (w0[t].x, c1, a0[t].y);
				a0[t].y = fmaf (w0[t].y, c2, a0[t].y);
				a1[t].x = fmaf (w1[t].x, h1.x, a1[t].x);
				a1[t].x = fmaf (-w1[t].y, h1.y, a1[t].x);
				a1[t].y = fmaf (w1[t].x, h1.y, a1[t].y);
				a1[t].y = fmaf (w1[t].y, h1.x, a1[t].y);
			}
#pragma unroll
			for (int t = CB_T - 1; t > 0; t--) {
				w0[t] = w0[t - 1];
				w1[t] = w1[t - 1];
			}
			w0[0] = x0; /* X_{b0-k-1} (unused after the last step) */
			w1[0] = x1;
		}
		/* pass 3: back to time, the mix, the stores; the drum samples and the mix in one round of loads */
		float dv[CB_T][2], mx[CB_T];
#pragma unroll
		for (int t = 0; t < CB_T; t++) {
			dv[t][0] = dv[t][1] = 0.0f;
			mx[t]    = mix0;
			if ((uint32_t)t < tn) {
				const float* d = drum + (uint64_t)(b0 + t) * TBF_CAB_PART;
				dv[t][0] = d[l];
				dv[t][1] = d[l + 64];
				if (P.wetBlk)
					mx[t] = P.wetBlk[(uint64_t)inst * nb + b0 + t];
			}
		}
#pragma unroll
		for (int t = 0; t < CB_T; t++) {
			if ((uint32_t)t >= tn)
				break;
			if (dc) {
				re[0]            = a0[t].x;
				im[0]            = 0.0f;
				re[cb_rev (128)] = a0[t].y;
				im[cb_rev (128)] = 0.0f;
			} else {
				const uint32_t p = cb_rev (l), q = cb_rev (256 - l);
				re[p] = a0[t].x;
				im[p] = a0[t].y;
				re[q] = a0[t].x;
				im[q] = -a0[t].y;
			}
			{
				const uint32_t p = cb_rev (l + 64), q = cb_rev (192 - l);
				re[p] = a1[t].x;
				im[p] = a1[t].y;
				re[q] = a1[t].x;
				im[q] = -a1[t].y;
			}
			__syncthreads ();
			float y[2];
			cb_ifft (re, im, twc, tws, W, y[0], y[1]);
			const float dry = __fsub_rn (1.0f, mx[t]);
#pragma unroll
			for (int q = 0; q < 2; q++) {
				const uint64_t s = (uint64_t)(b0 + t) * TBF_CAB_PART + l + 64 * q;
				const float    c = y[q] * (1.0f / TBF_CAB_FFT);
				out[s] = __fadd_rn (__fadd_rn (__fmul_rn (dry, hx[t][q]), __fmul_rn (mx[t], c)), dv[t][q]);
				if (wout)
					wout[s] = c;
			}
			__syncthreads ();
		}
		p0 = hx[CB_T - 1][0]; /* a full tile's last block; a short tile is the call's last */
		p1 = hx[CB_T - 1][1];
	}
	/* the state for the next call: the last block of horn samples, the next ring slot */
	if (nb) {
		const float* last = horn + (uint64_t)(nb - 1) * TBF_CAB_PART;
		tail[l]      = last[l];
		tail[l + 64] = last[l + 64];
		if (l == 0)
			*reinterpret_cast<uint32_t*> (S) = (pos + nb) % R;
	}
}

extern "C" int tbf_launch_cabinet (const tbf_cab_launch* P, hipStream_t stream)
{
	if (P->n == 0 || P->nb == 0)
		return 0;
	hipLaunchKernelGGL (k_cabinet, dim3 (2 * P->n), dim3 (64), 0, stream, *P);
	return hipGetLastError () == hipSuccess ? 0 : -5;
}
