/*
 * tbf_eq.h -- the arithmetic, constants and launch record of k_eq (csrc/tbf_eq.hip), shared with
 * its host side (csrc/tbf_eq.cpp) and with the host restatement tbf_debug_eq_ref, which runs the
 * same function; and eqCompute, the RBJ designer that the whirl's filters (csrc/tbf_init.cpp) and
 * the equaliser's bands both call.
 *
 * Definition (include/tbf.h, "Bus equaliser"): per row, channel and frame, v = (double) sample and,
 * for each band b = 0 .. nb - 1 in order with its five coefficients c = {b0, b1, b2, a1, a2}, every
 * operator one IEEE double operation,
 *     y = b0*v + s1;   s1 = (b1*v + s2) - a1*y;   s2 = b2*v - a2*y;   v = y           eq_step
 * and the output is (float) v.
 */
#ifndef TBF_EQ_H
#define TBF_EQ_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/tbf.h"

#define TBF_EQ_LANES 64u /* k_eq's workgroup: one wave */
#define TBF_EQ_TILE 128u /* frames of a row-channel staged in LDS at a time */
#define TBF_EQ_GROUP 4u  /* steps between two LDS reads of a lane: one ds_read_b128 */
/* floats between the row-channels of the LDS tile: 4 more than the tile, so that the 16-byte reads
 * of lanes that stand at the same frame of consecutive row-channels fall on different banks
 * (row-channel g at 4 g mod 64), as k_loud's */
#define TBF_EQ_PITCH (TBF_EQ_TILE + 4u)

#define TBF_EQ_MIN_RATE 8000u
#define TBF_EQ_MAX_RATE 192000u

#define TBF_EQ_HD __host__ __device__ __forceinline__

/* the lanes of a row-channel: the smallest of 1, 2, 4, 8 that holds max_bands (1..8) */
TBF_EQ_HD constexpr uint32_t eq_lanes (uint32_t max_bands) { return max_bands <= 1u ? 1u : max_bands <= 2u ? 2u : max_bands <= 4u ? 4u : 8u; }
/* the rows of a wave: both channels of 32 / P rows */
TBF_EQ_HD constexpr uint32_t eq_rows (uint32_t P) { return 32u / P; }
/* where row-channel g (< 64 / P) of the tile starts, in floats: the second 32 stand half a bank row
 * further, which puts row-channel g + 32 on the banks g + 8 would have (k_loud's planes) */
TBF_EQ_HD constexpr uint32_t eq_lds_off (uint32_t g) { return g * TBF_EQ_PITCH + (g >> 5) * 32u; }
TBF_EQ_HD constexpr uint32_t eq_lds_floats (uint32_t P) { return (64u / P) * TBF_EQ_PITCH + (P == 1u ? 32u : 0u); }

/* one frame through one band: v in, y out, the band's state replaced */
TBF_EQ_HD double eq_step (const double* c, double v, double& s1, double& s2)
{
	const double y = c[0] * v + s1;
	s1             = (c[1] * v + s2) - c[3] * y;
	s2             = c[2] * v - c[4] * y;
	return y;
}

typedef struct tbf_eq_launch {
	const float*    in[2];     /* the L / R rows */
	float*          out[2];
	uint64_t        inStride, outStride; /* floats between rows */
	const uint32_t* counts;    /* every row's frames of this call, or NULL: `frames` each */
	const uint32_t* nb;        /* [row]: the bands in use, <= maxBands */
	const double*   coef;      /* [row][maxBands][5]: b0, b1, b2, a1, a2 */
	double*         state;     /* [row][channel][maxBands][2]: s1, s2 */
	uint32_t        frames;
	uint32_t        maxBands;  /* 1..8 */
	uint32_t        nRows;
} tbf_eq_launch;

/* RBJ designer, src/eqcomp.cpp:98-203: the nine types LPF, HPF, BPF0, BPF1, notch, APF, PEQ, low
 * shelf, high shelf into C = {b0, b1, b2, a0, a1, a2}, all but a0 then divided by a0.  One function
 * for the whirl's filters and the equaliser's bands; the whirl's pins hold it to the reference. */
inline void eqCompute (int type, double fqHz, double Q, double dbG, double* C, double SampleRateD)
{
	double A = pow (10.0, (dbG / 40.0)), omega = (2.0 * M_PI * fqHz) / SampleRateD;
	double sin_ = sin (omega), cos_ = cos (omega), alpha = sin_ / (2.0 * Q), beta = sqrt (A) / Q;
	switch (type) {
		case 0: C[0] = (1.0 - cos_) / 2.0; C[1] = 1.0 - cos_; C[2] = (1.0 - cos_) / 2.0; C[3] = 1.0 + alpha; C[4] = -2.0 * cos_; C[5] = 1.0 - alpha; break;
		case 1: C[0] = (1.0 + cos_) / 2.0; C[1] = -(1.0 + cos_); C[2] = (1.0 + cos_) / 2.0; C[3] = 1.0 + alpha; C[4] = -2.0 * cos_; C[5] = 1.0 - alpha; break;
		case 2: C[0] = sin_ / 2.0; C[1] = 0.0; C[2] = -sin_ / 2.0; C[3] = 1.0 + alpha; C[4] = -2.0 * cos_; C[5] = 1.0 - alpha; break;
		case 3: C[0] = alpha; C[1] = 0.0; C[2] = -alpha; C[3] = 1.0 + alpha; C[4] = -2.0 * cos_; C[5] = 1.0 - alpha; break;
		case 4: C[0] = 1.0; C[1] = -2.0 * cos_; C[2] = 1.0; C[3] = 1.0 + alpha; C[4] = -2.0 * cos_; C[5] = 1.0 - alpha; break;
		case 5: C[0] = 1.0 - alpha; C[1] = -2.0 * cos_; C[2] = 1.0 + alpha; C[3] = 1.0 + alpha; C[4] = -2.0 * cos_; C[5] = 1.0 - alpha; break;
		case 6: C[0] = 1.0 + (alpha * A); C[1] = -2.0 * cos_; C[2] = 1.0 - (alpha * A); C[3] = 1.0 + (alpha / A); C[4] = -2.0 * cos_; C[5] = 1.0 - (alpha / A); break;
		case 7:
			C[0] = A * ((A + 1) - ((A - 1) * cos_) + (beta * sin_));
			C[1] = (2.0 * A) * ((A - 1) - ((A + 1) * cos_));
			C[2] = A * ((A + 1) - ((A - 1) * cos_) - (beta * sin_));
			C[3] = (A + 1) + ((A - 1) * cos_) + (beta * sin_);
			C[4] = -2.0 * ((A - 1) + ((A + 1) * cos_));
			C[5] = (A + 1) + ((A - 1) * cos_) - (beta * sin_);
			break;
		case 8:
			C[0] = A * ((A + 1) + ((A - 1) * cos_) + (beta * sin_));
			C[1] = -(2.0 * A) * ((A - 1) + ((A + 1) * cos_));
			C[2] = A * ((A + 1) + ((A - 1) * cos_) - (beta * sin_));
			C[3] = (A + 1) - ((A - 1) * cos_) + (beta * sin_);
			C[4] = 2.0 * ((A - 1) - ((A + 1) * cos_));
			C[5] = (A + 1) - ((A - 1) * cos_) - (beta * sin_);
			break;
	}
	C[0] /= C[3];
	C[1] /= C[3];
	C[2] /= C[3];
	C[4] /= C[3];
	C[5] /= C[3];
}

#endif
