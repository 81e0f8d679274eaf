/*
 * tbf_eq.cpp -- the host side of the bus equaliser: the equaliser objects an engine owns,
 * tbf_eq_device, set, reset, the read-back, and the tbf_debug_eq* hooks.
 *
 * A stage between two pairs of float32 device planes (include/tbf.h): k_eq
 * (csrc/tbf_eq.hip) runs every row's two channels through the row's own cascade of up to max_bands
 * biquads in double.  The coefficients are designed here, on the host, by eqCompute of
 * csrc/tbf_eq.h (the whirl's designer); the kernel receives them.  The host keeps every row's band
 * count and coefficients (tbf_eq.nb, .coef), which tbf_eq_set rewrites and uploads and
 * tbf_eq_bands reads back.  The state, two doubles per row, channel and band, belongs to the
 * equaliser, not to an instance: the render path, clone, save, load and remove do not know it.
 * Everything is checked before anything is staged or launched: a refused call writes nothing and
 * moves no state.  tbf_debug_eq_ref is the definition on the host, one row at a time, from eq_step
 * of csrc/tbf_eq.h, which the kernel runs.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_engine_impl.h"
#include "tbf_eq.h"

extern "C" int tbf_launch_eq (const tbf_eq_launch* A, hipStream_t stream);

using namespace tbf;

namespace {

int checkRate (uint32_t rate)
{
	if (rate < TBF_EQ_MIN_RATE || rate > TBF_EQ_MAX_RATE)
		return fail (-22, "eq: rate_hz " + std::to_string (rate) + " is not in [" + std::to_string (TBF_EQ_MIN_RATE) + ", " +
		                      std::to_string (TBF_EQ_MAX_RATE) + "]");
	return 0;
}

int checkMaxBands (uint32_t mb)
{
	if (mb < 1u || mb > TBF_EQ_MAX_BANDS)
		return fail (-22, "eq: max_bands " + std::to_string (mb) + " is not in [1, " + std::to_string (TBF_EQ_MAX_BANDS) + "]");
	return 0;
}

int checkConfig (const tbf_eq_config* cfg)
{
	if (!cfg)
		return fail (-22, "eq: cfg is NULL");
	if (int rc = checkRate (cfg->rate_hz))
		return rc;
	return checkMaxBands (cfg->max_bands);
}

/* setIIRFilter's guard, except the gain; a NaN fails every one of them.  `where` names the row and
 * the band in the error. */
int checkBand (const tbf_eq_band& bd, uint32_t rate, const std::string& where)
{
	if (bd.type < 0 || bd.type > 8)
		return fail (-22, "eq: " + where + ": type " + std::to_string (bd.type) + " is not in [0, 8]");
	if (!(bd.q > 0.1 && bd.q < 6.0))
		return fail (-22, "eq: " + where + ": q " + std::to_string (bd.q) + " is not inside (0.1, 6)");
	const double w = bd.hz / (double)rate;
	if (!(w > 0.0002 && w < 0.4998))
		return fail (-22, "eq: " + where + ": hz " + std::to_string (bd.hz) + " over the rate " + std::to_string (rate) +
		                      " is not inside (0.0002, 0.4998)");
	if (!(std::fabs (bd.gain_db) <= 24.0))
		return fail (-22, "eq: " + where + ": gain_db " + std::to_string (bd.gain_db) + " is not in [-24, 24]");
	return 0;
}

/* b0, b1, b2, a1, a2 of a checked band */
void design (const tbf_eq_band& bd, uint32_t rate, double* c5)
{
	double C[6];
	eqCompute (bd.type, bd.hz, bd.q, bd.gain_db, C, (double)rate);
	c5[0] = C[0], c5[1] = C[1], c5[2] = C[2], c5[3] = C[4], c5[4] = C[5];
}

std::string rowBand (uint32_t row, uint32_t band) { return "row " + std::to_string (row) + " band " + std::to_string (band); }

} // namespace

extern "C" {

int tbf_eq_create (tbf_engine* e, uint32_t n_rows, const tbf_eq_config* cfg, tbf_eq** out)
{
	if (!e)
		return fail (-22, "eq: engine is NULL");
	if (!out)
		return fail (-22, "eq: out is NULL");
	if (int rc = checkConfig (cfg))
		return rc;
	if (n_rows == 0)
		return fail (-22, "eq: n_rows is 0");
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) has no device to equalise on");
	HIPCHK (hipSetDevice (e->cfg.device));
	std::unique_ptr<tbf_eq> eq (new tbf_eq ());
	eq->eng   = e;
	eq->cfg   = *cfg;
	eq->nRows = n_rows;
	const size_t bands = (size_t)n_rows * cfg->max_bands;
	if (eq->state.ensure (bands * 4u) || eq->dcoef.ensure (bands * 5u) || eq->dnb.ensure (n_rows) || eq->dcounts.ensure (n_rows)) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (equaliser: 72 B per row and band, and 8 B per row)");
	}
	HIPCHK (hipMemsetAsync (eq->state.p, 0, bands * 4u * sizeof (double), e->stream));
	HIPCHK (hipMemsetAsync (eq->dcoef.p, 0, bands * 5u * sizeof (double), e->stream));
	HIPCHK (hipMemsetAsync (eq->dnb.p, 0, (size_t)n_rows * sizeof (uint32_t), e->stream));
	HIPCHK (hipStreamSynchronize (e->stream));
	eq->coef.assign (bands * 5u, 0.0);
	eq->nb.assign (n_rows, 0u);
	eq->counts.assign (n_rows, 0u);
	*out = eq.get ();
	e->eqs.push_back (std::move (eq));
	return 0;
}

int tbf_eq_destroy (tbf_eq* eq)
{
	if (!eq)
		return 0;
	auto it = slotOf (eq->eng->eqs, eq);
	if (it == eq->eng->eqs.end ())
		return fail (-22, "eq: not an equaliser of its engine");
	(void)hipSetDevice (eq->eng->cfg.device);
	eq->eng->eqs.erase (it); /* hipFree waits for the work that still uses the state */
	return 0;
}

int tbf_eq_reset (tbf_eq* eq, uint32_t n, const uint32_t* rows, void* stream)
{
	if (!eq)
		return fail (-22, "eq: eq is NULL");
	if (int rc = checkRows ("eq", n, rows, eq->nRows))
		return rc;
	HIPCHK (hipSetDevice (eq->eng->cfg.device));
	hipStream_t const s   = streamOr (stream, eq->eng->stream);
	const size_t      per = (size_t)eq->cfg.max_bands * 4u; /* a row's doubles: both channels, every band */
	if (!rows)
		HIPCHK (hipMemsetAsync (eq->state.p, 0, (size_t)eq->nRows * per * sizeof (double), s));
	for (uint32_t k = 0; rows && k < n; k++)
		HIPCHK (hipMemsetAsync (eq->state.p + (size_t)rows[k] * per, 0, per * sizeof (double), s));
	return 0;
}

int tbf_eq_set (tbf_eq* eq, uint32_t n, const uint32_t* rows, const tbf_eq_band* bands, const uint32_t* n_bands, void* stream)
{
	if (!eq)
		return fail (-22, "eq: eq is NULL");
	if (!n_bands)
		return fail (-22, "eq: n_bands is NULL");
	if (!rows)
		n = eq->nRows;
	if (int rc = checkRows ("eq", n, rows, eq->nRows))
		return rc;
	const uint32_t mb = eq->cfg.max_bands;
	size_t         total = 0;
	for (uint32_t k = 0; k < n; k++) {
		const uint32_t r = rows ? rows[k] : k;
		if (n_bands[k] > mb)
			return fail (-22, "eq: row " + std::to_string (r) + ": " + std::to_string (n_bands[k]) + " bands, max_bands is " +
			                      std::to_string (mb));
		if (n_bands[k] && !bands)
			return fail (-22, "eq: bands is NULL");
		for (uint32_t b = 0; b < n_bands[k]; b++)
			if (int rc = checkBand (bands[total + b], eq->cfg.rate_hz, rowBand (r, b)))
				return rc;
		total += n_bands[k];
	}
	HIPCHK (hipSetDevice (eq->eng->cfg.device));
	hipStream_t const s = streamOr (stream, eq->eng->stream);
	/* The host's tables first, then their rows to the device.  The copies read the equaliser's own
	 * vectors, which the next set rewrites, so the stream is waited for. */
	total = 0;
	for (uint32_t k = 0; k < n; k++) {
		const uint32_t r = rows ? rows[k] : k;
		for (uint32_t b = 0; b < n_bands[k]; b++)
			design (bands[total + b], eq->cfg.rate_hz, &eq->coef[((size_t)r * mb + b) * 5u]);
		eq->nb[r] = n_bands[k];
		total += n_bands[k];
	}
	const size_t per = (size_t)mb * 5u;
	if (!rows) {
		HIPCHK (hipMemcpyAsync (eq->dcoef.p, eq->coef.data (), (size_t)n * per * sizeof (double), hipMemcpyHostToDevice, s));
		HIPCHK (hipMemcpyAsync (eq->dnb.p, eq->nb.data (), (size_t)n * sizeof (uint32_t), hipMemcpyHostToDevice, s));
	}
	for (uint32_t k = 0; rows && k < n; k++) {
		const uint32_t r = rows[k];
		HIPCHK (hipMemcpyAsync (eq->dcoef.p + (size_t)r * per, &eq->coef[(size_t)r * per], per * sizeof (double), hipMemcpyHostToDevice, s));
		HIPCHK (hipMemcpyAsync (eq->dnb.p + r, &eq->nb[r], sizeof (uint32_t), hipMemcpyHostToDevice, s));
	}
	HIPCHK (hipStreamSynchronize (s));
	return 0;
}

int tbf_eq_bands (const tbf_eq* eq, uint32_t row, double* coeffs, uint32_t cap, uint32_t* nb)
{
	if (!eq)
		return fail (-22, "eq: eq is NULL");
	if (!nb)
		return fail (-22, "eq: nb is NULL");
	if (row >= eq->nRows)
		return fail (-22, "eq: row " + std::to_string (row) + " is no row of n_rows " + std::to_string (eq->nRows));
	const uint32_t N = eq->nb[row];
	*nb              = N;
	if (N > cap)
		return fail (-28, "eq: " + std::to_string (N) + " bands, cap is " + std::to_string (cap));
	if (N && !coeffs)
		return fail (-22, "eq: coeffs is NULL");
	if (N)
		memcpy (coeffs, &eq->coef[(size_t)row * eq->cfg.max_bands * 5u], (size_t)N * 5u * sizeof (double));
	return 0;
}

int tbf_eq_device (tbf_eq* eq, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames, float* d_outL, float* d_outR,
                   uint64_t out_stride, const uint32_t* counts, void* stream)
{
	if (!eq)
		return fail (-22, "eq: eq is NULL");
	if (!d_L || !d_R)
		return fail (-22, std::string ("eq: ") + (d_L ? "d_R" : "d_L") + " is NULL");
	if (!d_outL || !d_outR)
		return fail (-22, std::string ("eq: ") + (d_outL ? "d_outR" : "d_outL") + " is NULL");
	if (in_stride < frames)
		return fail (-22, "eq: in_stride smaller than frames");
	if (out_stride < frames)
		return fail (-22, "eq: out_stride smaller than frames");
	if (((uintptr_t)d_L | (uintptr_t)d_R | (uintptr_t)d_outL | (uintptr_t)d_outR) & 3u)
		return fail (-22, "eq: device pointer not 4-byte aligned");
	const uint32_t n = eq->nRows;
	uint32_t       most;
	if (int rc = countsMost ("eq", counts, n, frames, &most))
		return rc;
	{
		const uint64_t rowBytes = (uint64_t)frames * 4;
		const Span     sp[4]    = {rowsSpan (d_L, n, in_stride * 4, rowBytes), rowsSpan (d_R, n, in_stride * 4, rowBytes),
		                           rowsSpan (d_outL, n, out_stride * 4, rowBytes), rowsSpan (d_outR, n, out_stride * 4, rowBytes)};
		if (anyOverlap (sp, 4, 2)) /* d_L and d_R may be one plane: mono */
			return fail (-22, "eq: input rows and output planes overlap (in-place use is refused)");
	}
	tbf_engine* const e = eq->eng;
	HIPCHK (hipSetDevice (e->cfg.device));
	hipStream_t const s = streamOr (stream, e->stream);
	if (most == 0)
		return 0;
	/* The counts on the device.  They are read from the equaliser's host vector, which the next
	 * call rewrites, so the stream is waited for.  A call without counts uploads nothing. */
	if (counts) {
		std::copy (counts, counts + n, eq->counts.begin ());
		HIPCHK (hipMemcpyAsync (eq->dcounts.p, eq->counts.data (), (size_t)n * sizeof (uint32_t), hipMemcpyHostToDevice, s));
		HIPCHK (hipStreamSynchronize (s));
	}

	tbf_eq_launch A;
	memset (&A, 0, sizeof (A));
	A.in[0]     = d_L;
	A.in[1]     = d_R;
	A.out[0]    = d_outL;
	A.out[1]    = d_outR;
	A.inStride  = in_stride;
	A.outStride = out_stride;
	A.counts    = counts ? eq->dcounts.p : nullptr;
	A.nb        = eq->dnb.p;
	A.coef      = eq->dcoef.p;
	A.state     = eq->state.p;
	A.frames    = frames;
	A.maxBands  = eq->cfg.max_bands;
	A.nRows     = n;

	StageTimer::Guard tg (eq->timer, s, "eq"); /* tbf_debug_eq_time: the launch between two events on its stream */
	if (int rc = tg.begin ())
		return rc;
	if (tbf_launch_eq (&A, s))
		return fail (-5, std::string ("k_eq launch failed: ") + hipGetErrorString (hipGetLastError ()));
	return tg.end ();
}

int tbf_debug_eq_coeffs (uint32_t rate_hz, const tbf_eq_band* band, double* c5)
{
	if (int rc = checkRate (rate_hz))
		return rc;
	if (!band)
		return fail (-22, "eq: band is NULL");
	if (!c5)
		return fail (-22, "eq: c5 is NULL");
	if (int rc = checkBand (*band, rate_hz, rowBand (0u, 0u)))
		return rc;
	design (*band, rate_hz, c5);
	return 0;
}

int tbf_debug_eq_ref (const double* coeffs, uint32_t nb, const float* L, const float* R, uint64_t n, double* state, float* outL,
                      float* outR)
{
	if (nb > TBF_EQ_MAX_BANDS)
		return fail (-22, "eq: " + std::to_string (nb) + " bands, the most is " + std::to_string (TBF_EQ_MAX_BANDS));
	if (nb && (!coeffs || !state))
		return fail (-22, std::string ("eq: ") + (coeffs ? "state" : "coeffs") + " is NULL");
	if (n && (!L || !R || !outL || !outR))
		return fail (-22, "eq: a plane is NULL");
	for (int ch = 0; ch < 2; ch++) {
		const float* x  = ch ? R : L;
		float*       o  = ch ? outR : outL;
		double*      st = state + (size_t)ch * nb * 2u;
		for (uint64_t i = 0; i < n; i++) {
			double v = (double)x[i];
			for (uint32_t b = 0; b < nb; b++)
				v = eq_step (coeffs + 5u * b, v, st[2u * b], st[2u * b + 1u]);
			o[i] = (float)v;
		}
	}
	return 0;
}

int tbf_debug_eq_grid (uint32_t max_bands, uint32_t* lanes, uint32_t* rows_per_wave, uint32_t* tile_frames, uint32_t* lds_bytes)
{
	if (int rc = checkMaxBands (max_bands))
		return rc;
	const uint32_t P = eq_lanes (max_bands);
	if (lanes)
		*lanes = P;
	if (rows_per_wave)
		*rows_per_wave = eq_rows (P);
	if (tile_frames)
		*tile_frames = TBF_EQ_TILE;
	if (lds_bytes)
		*lds_bytes = ((eq_lds_floats (P) + 3u) / 4u) * 16u;
	return 0;
}

int tbf_debug_eq_time (tbf_eq* eq, int32_t enable, double* ms, uint64_t* launches)
{
	if (!eq)
		return fail (-22, "eq: eq is NULL");
	return eq->timer.query (enable, ms, launches);
}

} /* extern "C" */
