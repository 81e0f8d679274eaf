/*
 * tbf_cabinet.h -- the layout and launch record of k_cabinet (csrc/tbf_cabinet.hip), shared
 * with its host side (csrc/tbf_cabinet.cpp).
 *
 * Uniformly partitioned overlap-save at the block size: partition 128, FFT 256.  A spectrum is
 * stored packed, 128 complex floats: bin 0 holds (Re X[0], Re X[128]), both real for a real
 * signal, bins 1 .. 127 as they are.
 * Per instance and channel the state is TBF_CAB_HDR + 128 + R * 256 floats:
 *   [0]            (uint32) the ring slot of the next block's spectrum
 *   [4, 132)       the last block of horn samples (the first half of the next FFT frame)
 *   [132, ...)     a ring of R = K + TBF_CAB_TILE - 1 packed spectra of the last blocks
 * (K = ceil (taps / 128) partitions; the TBF_CAB_TILE - 1 extra slots let a tile of blocks
 * store its spectra before the oldest ones it still reads are overwritten).
 */
#ifndef TBF_CABINET_H
#define TBF_CABINET_H

#include <stdint.h>

#define TBF_CAB_PART 128 /* partition = block size */
#define TBF_CAB_FFT 256
#define TBF_CAB_TILE 8   /* output blocks per pass over the response's spectra */
#define TBF_CAB_HDR 4    /* floats in front of a channel's tail and ring */

#define TBF_CAB_RING(K) ((K) + TBF_CAB_TILE - 1)
#define TBF_CAB_CH_FLOATS(K) ((uint64_t)TBF_CAB_HDR + TBF_CAB_PART + (uint64_t)TBF_CAB_RING (K) * TBF_CAB_FFT)

typedef struct tbf_cab_launch {
	const float* horn[2];   /* hornL, hornR rows */
	const float* drum[2];   /* drumL, drumR rows */
	uint64_t     rotStride; /* floats between instances of the four */
	float*       out[2];    /* (dry * horn + wet * conv) + drum */
	float*       wet[2];    /* the convolver's own output, or NULL */
	uint64_t     outStride;
	float*       state;     /* instance i, channel c at state + (2 i + c) * chFloats */
	uint64_t     chFloats;
	const float* H[2];      /* the response's packed spectra, [K][128] complex, per channel */
	const float* tw;        /* exp (-2 pi i j / 256), j = 0 .. 127: 128 cosines, then 128 sines (negated) */
	const float* wet0;      /* the mix per instance ... */
	const float* wetBlk;    /* ... or, when a mix event lands in the call, per (instance, block); else NULL */
	uint32_t     n, nb;     /* instances, blocks */
	uint32_t     K, R;      /* partitions, ring slots */
} tbf_cab_launch;

#endif
