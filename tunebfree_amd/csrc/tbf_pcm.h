/*
 * tbf_pcm.h -- the arithmetic, packing and launch record of k_pcm (csrc/tbf_pcm.hip), shared with
 * its host side (csrc/tbf_pcm.cpp) and with the host restatement tbf_debug_pcm_ref, which runs the
 * same functions.
 *
 * Definition (include/tbf.h): per float32 sample x and scale S (32768 for S16, 8388608 for S24)
 *     v = x * S;  t = v, or v + d under TBF_PCM_DITHER;  q = rintf (t), ties to even;
 *     NaN -> 0, q > max -> max, q < min -> min, each counted as a clip,
 * one float32 operation per step, denormals kept.  F32 copies the sample's bits and counts
 * !(|x| <= 1).  d is TPDF dither of +-1 LSB from a counter hash of (seed, row, channel, frame).
 * A frame is L then R; frames are packed back to back, little-endian.
 *
 * The unit of work is a group of up to four frames that starts at a frame index divisible by
 * four: pcm_group turns it into up to eight dwords, which are whole in every format except for
 * the 2-byte tail behind an odd number of S24 frames.
 */
#ifndef TBF_PCM_H
#define TBF_PCM_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/tbf.h"

#define TBF_PCM_LANES 256u      /* k_pcm's workgroup */
#define TBF_PCM_GROUP 4u        /* frames a lane carries */
#define TBF_PCM_TILE (TBF_PCM_LANES * TBF_PCM_GROUP)
#define TBF_PCM_MAX_ROWS 65535u /* rows of one launch (the grid's y) */

#define TBF_PCM_HD __host__ __device__ __forceinline__

TBF_PCM_HD uint32_t pcm_frame_bytes (uint32_t fmt) { return fmt == TBF_PCM_S16 ? 4u : fmt == TBF_PCM_S24_3LE ? 6u : 8u; }

TBF_PCM_HD float pcm_float (uint32_t b)
{
	float f;
	__builtin_memcpy (&f, &b, 4);
	return f;
}

TBF_PCM_HD uint32_t pcm_bits (float f)
{
	uint32_t b;
	__builtin_memcpy (&b, &f, 4);
	return b;
}

/* h (a), the 32-bit mixer */
TBF_PCM_HD uint32_t pcm_hash (uint32_t a)
{
	a ^= a >> 16;
	a *= 0x7feb352du;
	a ^= a >> 15;
	a *= 0x846ca68bu;
	a ^= a >> 16;
	return a;
}

/* d of row r, channel c, frame f: the difference of two 16-bit uniforms, in LSBs */
TBF_PCM_HD float pcm_dither (uint32_t seed, uint32_t r, uint32_t c, uint64_t f)
{
	const uint32_t k = pcm_hash (pcm_hash (pcm_hash (seed ^ (2u * r + c)) ^ (uint32_t)f) ^ (uint32_t)(f >> 32));
	return ((float)(k & 0xffffu) - (float)(k >> 16)) * 0x1p-16f;
}

/* a row's meter as the lanes carry it: the peak as the bits of a non-negative float (they order
 * as the floats do), the clip count */
struct pcm_acc {
	uint32_t peak[2], clip[2];
};

TBF_PCM_HD void pcm_peak (float x, uint32_t& peak)
{
	const float a = fabsf (x);
	if (a == a && pcm_bits (a) > peak) /* NaN is skipped */
		peak = pcm_bits (a);
}

/* one sample to an integer of [lo, hi] */
template <bool DITHER>
TBF_PCM_HD int32_t pcm_quant (float x, float S, float hi, float lo, float d, uint32_t& clip)
{
	const float v = x * S;
	const float t = DITHER ? v + d : v;
	float       q = rintf (t);
	if (!(q == q)) {
		q = 0.0f;
		clip++;
	} else if (q > hi) {
		q = hi;
		clip++;
	} else if (q < lo) {
		q = lo;
		clip++;
	}
	return (int32_t)q;
}

/* Frames j .. j + nf - 1 (nf 1 .. 4) of row `row`, their samples' bits in l[] / r[], the first at
 * dither frame f: the packed bytes as little-endian dwords in w[], metered into m.  Returns the
 * byte count nf * frame bytes: the dwords below it are whole, and when it is no multiple of 4
 * (S24, nf odd) the low half of the next dword is the 2-byte tail. */
template <int FMT, bool DITHER>
TBF_PCM_HD uint32_t pcm_group (const uint32_t (&l)[4], const uint32_t (&r)[4], uint32_t nf, uint32_t seed, uint32_t row,
                               uint64_t f, uint32_t (&w)[8], pcm_acc& m)
{
	if (FMT == TBF_PCM_F32) {
#pragma unroll
		for (uint32_t k = 0; k < 4; k++) {
			const bool on = k < nf;
			w[2 * k]      = on ? l[k] : 0u;
			w[2 * k + 1]  = on ? r[k] : 0u;
			if (on) {
				const float xl = pcm_float (l[k]), xr = pcm_float (r[k]);
				pcm_peak (xl, m.peak[0]);
				pcm_peak (xr, m.peak[1]);
				m.clip[0] += !(fabsf (xl) <= 1.0f);
				m.clip[1] += !(fabsf (xr) <= 1.0f);
			}
		}
		return nf * 8u;
	}
	const bool  s16 = FMT == TBF_PCM_S16;
	const float S = s16 ? 32768.0f : 8388608.0f, hi = s16 ? 32767.0f : 8388607.0f, lo = -S;
	uint32_t    s[8];
#pragma unroll
	for (uint32_t k = 0; k < 4; k++) {
		s[2 * k] = s[2 * k + 1] = 0u;
		if (k < nf) {
			const float xl = pcm_float (l[k]), xr = pcm_float (r[k]);
			pcm_peak (xl, m.peak[0]);
			pcm_peak (xr, m.peak[1]);
			const float dl = DITHER ? pcm_dither (seed, row, 0u, f + k) : 0.0f;
			const float dr = DITHER ? pcm_dither (seed, row, 1u, f + k) : 0.0f;
			s[2 * k]       = (uint32_t)pcm_quant<DITHER> (xl, S, hi, lo, dl, m.clip[0]) & (s16 ? 0xffffu : 0xffffffu);
			s[2 * k + 1]   = (uint32_t)pcm_quant<DITHER> (xr, S, hi, lo, dr, m.clip[1]) & (s16 ? 0xffffu : 0xffffffu);
		}
	}
	if (s16) {
#pragma unroll
		for (uint32_t k = 0; k < 4; k++) {
			w[k]     = s[2 * k] | (s[2 * k + 1] << 16);
			w[k + 4] = 0u;
		}
		return nf * 4u;
	}
	/* four 3-byte samples into three dwords, twice */
#pragma unroll
	for (uint32_t h = 0; h < 2; h++) {
		const uint32_t a = s[4 * h], b = s[4 * h + 1], c = s[4 * h + 2], d = s[4 * h + 3];
		w[3 * h]         = a | (b << 24);
		w[3 * h + 1]     = (b >> 8) | (c << 16);
		w[3 * h + 2]     = (c >> 16) | (d << 8);
	}
	w[6] = w[7] = 0u;
	return nf * 6u;
}

/* a row's count and first dither frame, where they differ between rows */
typedef struct tbf_pcm_row {
	uint64_t frame0;
	uint32_t count;
	uint32_t pad;
} tbf_pcm_row;

typedef struct tbf_pcm_launch {
	const float*       in[2];     /* the L / R rows */
	uint64_t           inStride;  /* floats between rows */
	unsigned char*     out;       /* row r's frames from out + r * outStride */
	uint64_t           outStride; /* bytes between rows */
	tbf_pcm_meter*     meters;    /* one per row, zeroed by the caller, or NULL */
	const tbf_pcm_row* rows;      /* per row, or NULL; its counts hold when rowCounts, its frame0 always */
	uint64_t           frame0U;   /* without rows: every row's first dither frame */
	uint64_t           frameOff;  /* added to a row's frame0: the piece's place in its call */
	uint32_t           countU;    /* without rowCounts: every row's count */
	uint32_t           rowCounts;
	uint32_t           nRows, rowBase; /* rows of this launch (<= TBF_PCM_MAX_ROWS), the first one's number */
	uint32_t           maxCount;  /* the largest count: the grid's x covers it */
	uint32_t           format, flags, seed;
} tbf_pcm_launch;

#endif
