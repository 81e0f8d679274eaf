/*
 * tbf_loud.h -- the arithmetic, constants and launch record of k_loud (csrc/tbf_loud.hip), shared
 * with its host side (csrc/tbf_loud.cpp) and with the host restatement tbf_debug_loudness_ref,
 * which runs the same function.
 *
 * Definition (include/tbf.h, "Loudness meter"): per row and channel, with the seven coefficients
 * c = {b0, b1, b2, a1, a2, c1, c2} and x = (double) sample, every operator one IEEE double operation,
 *     y  = b0*x + s1;   s1 = (b1*x + s2) - a1*y;    s2 = b2*x - a2*y         the shelf
 *     w  = y + t1;      t1 = (-2.0*y + t2) - c1*w;  t2 = y - c2*w            the high-pass
 *     acc = acc + w*w;  k = k + 1                                             loud_step
 * and, once k == Hp, the hop's energy is acc, and acc and k start again from zero.
 */
#ifndef TBF_LOUD_H
#define TBF_LOUD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tbf.h"

#define TBF_LOUD_LANES 64u  /* k_loud's workgroup: one wave */
#define TBF_LOUD_ROWS 32u   /* rows of a workgroup: lane l walks row l % 32, channel l / 32 */
#define TBF_LOUD_TILE 128u  /* frames of a row staged in LDS at a time */
#define TBF_LOUD_GROUP 4u   /* frames a lane reads from LDS at a time: one ds_read_b128 */
/* floats between the rows of the LDS tile: 4 more than the tile, so that the 16-byte reads of
 * lanes that stand at the same frame of consecutive rows fall on different banks (row r at
 * 4 r mod 64) */
#define TBF_LOUD_PITCH (TBF_LOUD_TILE + 4u)
/* floats between the two channels' halves of the tile: 32 rows and half a bank row, which puts
 * lane l + 32 on the banks lane l + 8 would have */
#define TBF_LOUD_PLANE (TBF_LOUD_ROWS * TBF_LOUD_PITCH + 32u)
#define TBF_LOUD_LDS_BYTES (2u * TBF_LOUD_PLANE * 4u)

#define TBF_LOUD_MIN_RATE 8000u
#define TBF_LOUD_MAX_RATE 192000u

#define TBF_LOUD_HD __host__ __device__ __forceinline__

/* one channel of a row: 48 B, in registers for the length of a call */
typedef struct tbf_loud_chan {
	double   s1, s2, t1, t2, acc;
	uint32_t k;   /* frames of the open hop, < Hp */
	uint32_t hop; /* complete hops */
} tbf_loud_chan;

/* one frame through both biquads into the hop's sum; the caller tests k against Hp */
TBF_LOUD_HD void loud_step (const double* c, double x, tbf_loud_chan& S)
{
	const double y = c[0] * x + S.s1;
	S.s1           = (c[1] * x + S.s2) - c[3] * y;
	S.s2           = c[2] * x - c[4] * y;
	const double w = y + S.t1;
	S.t1           = (-2.0 * y + S.t2) - c[5] * w;
	S.t2           = y - c[6] * w;
	S.acc          = S.acc + w * w;
	S.k            = S.k + 1u;
}

typedef struct tbf_loud_launch {
	const float*    in[2];    /* the L / R rows */
	uint64_t        inStride; /* floats between rows */
	const uint32_t* counts;   /* every row's frames of this call */
	tbf_loud_chan*  state;    /* [row][channel] */
	double*         energy;   /* [row][hop][channel], maxHops hops a row */
	double          c[7];
	uint32_t        Hp, maxHops;
	uint32_t        nRows;
} tbf_loud_launch;

#endif
