/*
 * tbf_comp.cpp -- the host side of the bus compressor: the compressor objects an engine owns,
 * tbf_comp_device, the setters, reset, the read-back, the curve designer, and the tbf_debug_comp*
 * hooks.
 *
 * A stage between two pairs of float32 device planes (include/tbf.h): k_comp
 * (csrc/tbf_comp.hip) runs every row's gain behind a target that it reads from one of the
 * compressor's curves.  A curve is 769 points of data: tbf_comp_curve_design makes one here, on
 * the host, in double with libm; the kernel receives points and never derives them.  The host keeps
 * the curves and every row's parameters (tbf_comp.curves, .rows), which the setters rewrite and
 * upload and the getters read back.  The state, one float per row, belongs to the compressor, not
 * to an instance: the render path, clone, save, load and remove do not know it.  Everything is
 * checked before anything is staged or launched: a refused call writes nothing and moves no state.
 * tbf_debug_comp_ref is the definition on the host, one row at a time, from comp_lookup, comp_step
 * and comp_out of csrc/tbf_comp.h, which the kernel runs.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_comp.h"
#include "tbf_engine_impl.h"

extern "C" int tbf_launch_comp (const tbf_comp_launch* A, hipStream_t stream);

using namespace tbf;

namespace {

int checkCurves (uint32_t nc)
{
	if (nc < 1u || nc > TBF_COMP_MAX_CURVES)
		return fail (-22, "comp: n_curves " + std::to_string (nc) + " is not in [1, " + std::to_string (TBF_COMP_MAX_CURVES) + "]");
	return 0;
}

/* every point finite and in [0, 1]; a NaN fails the test, and so does -0.0f, whose bits are not
 * among those of [0, 1]: with it a gain could be -0.0f, and the meter's minimum orders bit patterns */
int checkPoints (const float* pts)
{
	for (uint32_t i = 0; i < TBF_COMP_POINTS; i++)
		if (!(pts[i] >= 0.0f && pts[i] <= 1.0f) || std::signbit (pts[i]))
			return fail (-22, "comp: point " + std::to_string (i) + ": " + std::to_string (pts[i]) + " is not in [0, 1]");
	return 0;
}

/* a row's parameters; a NaN fails every test.  n_curves 0: the curve index is not looked at. */
int checkRow (const tbf_comp_row& p, uint32_t n_curves, uint32_t row)
{
	const std::string where = "comp: row " + std::to_string (row) + ": ";
	if (n_curves && p.curve >= n_curves)
		return fail (-22, where + "curve " + std::to_string (p.curve) + " is no curve of n_curves " + std::to_string (n_curves));
	if (!(p.attack >= 0.0f && p.attack < 1.0f))
		return fail (-22, where + "attack " + std::to_string (p.attack) + " is not in [0, 1)");
	if (!(p.release >= 0.0f && p.release < 1.0f))
		return fail (-22, where + "release " + std::to_string (p.release) + " is not in [0, 1)");
	if (!(p.makeup >= 0.0f && p.makeup <= TBF_COMP_MAX_MAKEUP))
		return fail (-22, where + "makeup " + std::to_string (p.makeup) + " is not in [0, " + std::to_string ((int)TBF_COMP_MAX_MAKEUP) + "]");
	return 0;
}

} // namespace

extern "C" {

int tbf_comp_create (tbf_engine* e, uint32_t n_rows, const tbf_comp_config* cfg, tbf_comp** out)
{
	if (!e)
		return fail (-22, "comp: engine is NULL");
	if (!out)
		return fail (-22, "comp: out is NULL");
	if (!cfg)
		return fail (-22, "comp: cfg is NULL");
	if (int rc = checkCurves (cfg->n_curves))
		return rc;
	if (n_rows == 0)
		return fail (-22, "comp: n_rows is 0");
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) has no device to compress on");
	HIPCHK (hipSetDevice (e->cfg.device));
	std::unique_ptr<tbf_comp> cp (new tbf_comp ());
	cp->eng         = e;
	cp->cfg         = *cfg;
	cp->nRows       = n_rows;
	const size_t pts = (size_t)cfg->n_curves * TBF_COMP_POINTS;
	if (cp->state.ensure (n_rows) || cp->dcurves.ensure (pts) || cp->drows.ensure (n_rows) || cp->dcounts.ensure (n_rows)) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (compressor: 24 B per row, and 3076 B per curve)");
	}
	cp->curves.assign (pts, 1.0f);
	cp->rows.assign (n_rows, tbf_comp_row{0u, 0.0f, 0.0f, 1.0f});
	cp->ones.assign (n_rows, 1.0f);
	cp->counts.assign (n_rows, 0u);
	HIPCHK (hipMemcpyAsync (cp->state.p, cp->ones.data (), (size_t)n_rows * sizeof (float), hipMemcpyHostToDevice, e->stream));
	HIPCHK (hipMemcpyAsync (cp->dcurves.p, cp->curves.data (), pts * sizeof (float), hipMemcpyHostToDevice, e->stream));
	HIPCHK (hipMemcpyAsync (cp->drows.p, cp->rows.data (), (size_t)n_rows * sizeof (tbf_comp_row), hipMemcpyHostToDevice, e->stream));
	HIPCHK (hipStreamSynchronize (e->stream));
	*out = cp.get ();
	e->comps.push_back (std::move (cp));
	return 0;
}

int tbf_comp_destroy (tbf_comp* cp)
{
	if (!cp)
		return 0;
	auto it = slotOf (cp->eng->comps, cp);
	if (it == cp->eng->comps.end ())
		return fail (-22, "comp: not a compressor of its engine");
	(void)hipSetDevice (cp->eng->cfg.device);
	cp->eng->comps.erase (it); /* hipFree waits for the work that still uses the state */
	return 0;
}

int tbf_comp_reset (tbf_comp* cp, uint32_t n, const uint32_t* rows, void* stream)
{
	if (!cp)
		return fail (-22, "comp: comp is NULL");
	if (int rc = checkRows ("comp", n, rows, cp->nRows))
		return rc;
	HIPCHK (hipSetDevice (cp->eng->cfg.device));
	hipStream_t const s = streamOr (stream, cp->eng->stream);
	/* from `ones`, which nothing rewrites while the compressor lives: no wait */
	if (!rows)
		HIPCHK (hipMemcpyAsync (cp->state.p, cp->ones.data (), (size_t)cp->nRows * sizeof (float), hipMemcpyHostToDevice, s));
	for (uint32_t k = 0; rows && k < n; k++)
		HIPCHK (hipMemcpyAsync (cp->state.p + rows[k], cp->ones.data (), sizeof (float), hipMemcpyHostToDevice, s));
	return 0;
}

int tbf_comp_curve_set (tbf_comp* cp, uint32_t curve, const float* pts, void* stream)
{
	if (!cp)
		return fail (-22, "comp: comp is NULL");
	if (!pts)
		return fail (-22, "comp: pts is NULL");
	if (curve >= cp->cfg.n_curves)
		return fail (-22, "comp: curve " + std::to_string (curve) + " is no curve of n_curves " + std::to_string (cp->cfg.n_curves));
	if (int rc = checkPoints (pts))
		return rc;
	HIPCHK (hipSetDevice (cp->eng->cfg.device));
	hipStream_t const s  = streamOr (stream, cp->eng->stream);
	const size_t      at = (size_t)curve * TBF_COMP_POINTS;
	/* The host's table first, then the curve to the device.  The copy reads the compressor's own
	 * vector, which the next set rewrites, so the stream is waited for. */
	std::copy (pts, pts + TBF_COMP_POINTS, cp->curves.begin () + at);
	HIPCHK (hipMemcpyAsync (cp->dcurves.p + at, &cp->curves[at], TBF_COMP_POINTS * sizeof (float), hipMemcpyHostToDevice, s));
	HIPCHK (hipStreamSynchronize (s));
	return 0;
}

int tbf_comp_rows_set (tbf_comp* cp, uint32_t n, const uint32_t* rows, const tbf_comp_row* params, void* stream)
{
	if (!cp)
		return fail (-22, "comp: comp is NULL");
	if (!params)
		return fail (-22, "comp: params is NULL");
	if (!rows)
		n = cp->nRows;
	if (int rc = checkRows ("comp", n, rows, cp->nRows))
		return rc;
	for (uint32_t k = 0; k < n; k++)
		if (int rc = checkRow (params[k], cp->cfg.n_curves, rows ? rows[k] : k))
			return rc;
	HIPCHK (hipSetDevice (cp->eng->cfg.device));
	hipStream_t const s = streamOr (stream, cp->eng->stream);
	for (uint32_t k = 0; k < n; k++)
		cp->rows[rows ? rows[k] : k] = params[k];
	if (!rows)
		HIPCHK (hipMemcpyAsync (cp->drows.p, cp->rows.data (), (size_t)n * sizeof (tbf_comp_row), hipMemcpyHostToDevice, s));
	for (uint32_t k = 0; rows && k < n; k++)
		HIPCHK (hipMemcpyAsync (cp->drows.p + rows[k], &cp->rows[rows[k]], sizeof (tbf_comp_row), hipMemcpyHostToDevice, s));
	HIPCHK (hipStreamSynchronize (s));
	return 0;
}

int tbf_comp_curve_get (const tbf_comp* cp, uint32_t curve, float* pts)
{
	if (!cp)
		return fail (-22, "comp: comp is NULL");
	if (!pts)
		return fail (-22, "comp: pts is NULL");
	if (curve >= cp->cfg.n_curves)
		return fail (-22, "comp: curve " + std::to_string (curve) + " is no curve of n_curves " + std::to_string (cp->cfg.n_curves));
	memcpy (pts, &cp->curves[(size_t)curve * TBF_COMP_POINTS], TBF_COMP_POINTS * sizeof (float));
	return 0;
}

int tbf_comp_row_get (const tbf_comp* cp, uint32_t row, tbf_comp_row* out)
{
	if (!cp)
		return fail (-22, "comp: comp is NULL");
	if (!out)
		return fail (-22, "comp: out is NULL");
	if (row >= cp->nRows)
		return fail (-22, "comp: row " + std::to_string (row) + " is no row of n_rows " + std::to_string (cp->nRows));
	*out = cp->rows[row];
	return 0;
}

int tbf_comp_device (tbf_comp* cp, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames, const float* d_keyL,
                     const float* d_keyR, uint64_t key_stride, float* d_outL, float* d_outR, uint64_t out_stride, const uint32_t* counts,
                     tbf_comp_meter* d_meters, void* stream)
{
	if (!cp)
		return fail (-22, "comp: comp is NULL");
	if (!d_L || !d_R)
		return fail (-22, std::string ("comp: ") + (d_L ? "d_R" : "d_L") + " is NULL");
	if (!d_outL || !d_outR)
		return fail (-22, std::string ("comp: ") + (d_outL ? "d_outR" : "d_outL") + " is NULL");
	if ((d_keyL == nullptr) != (d_keyR == nullptr))
		return fail (-22, std::string ("comp: ") + (d_keyL ? "d_keyR" : "d_keyL") + " is NULL and the other key plane is not");
	if (in_stride < frames)
		return fail (-22, "comp: in_stride smaller than frames");
	if (d_keyL && key_stride < frames)
		return fail (-22, "comp: key_stride smaller than frames");
	if (out_stride < frames)
		return fail (-22, "comp: out_stride smaller than frames");
	if (((uintptr_t)d_L | (uintptr_t)d_R | (uintptr_t)d_keyL | (uintptr_t)d_keyR | (uintptr_t)d_outL | (uintptr_t)d_outR | (uintptr_t)d_meters) & 3u)
		return fail (-22, "comp: device pointer not 4-byte aligned");
	const uint32_t n = cp->nRows;
	uint32_t       most;
	if (int rc = countsMost ("comp", counts, n, frames, &most))
		return rc;
	{
		const uint64_t rowBytes = (uint64_t)frames * 4;
		const Span     sp[6]    = {rowsSpan (d_L, n, in_stride * 4, rowBytes),      rowsSpan (d_R, n, in_stride * 4, rowBytes),
		                           rowsSpan (d_keyL, n, key_stride * 4, rowBytes),  rowsSpan (d_keyR, n, key_stride * 4, rowBytes),
		                           rowsSpan (d_outL, n, out_stride * 4, rowBytes),  rowsSpan (d_outR, n, out_stride * 4, rowBytes)};
		if (anyOverlap (sp, 6, 4)) /* the inputs and the key may be one plane */
			return fail (-22, "comp: input or key rows and output planes overlap (in-place use is refused)");
	}
	tbf_engine* const e = cp->eng;
	HIPCHK (hipSetDevice (e->cfg.device));
	hipStream_t const s = streamOr (stream, e->stream);
	if (most == 0 && !d_meters)
		return 0;
	/* The counts on the device.  They are read from the compressor's host vector, which the next
	 * call rewrites, so the stream is waited for.  A call without counts uploads nothing. */
	if (counts) {
		std::copy (counts, counts + n, cp->counts.begin ());
		HIPCHK (hipMemcpyAsync (cp->dcounts.p, cp->counts.data (), (size_t)n * sizeof (uint32_t), hipMemcpyHostToDevice, s));
		HIPCHK (hipStreamSynchronize (s));
	}

	tbf_comp_launch A;
	memset (&A, 0, sizeof (A));
	A.in[0]       = d_L;
	A.in[1]       = d_R;
	A.key[0]      = d_keyL;
	A.key[1]      = d_keyR;
	A.out[0]      = d_outL;
	A.out[1]      = d_outR;
	A.inStride    = in_stride;
	A.keyStride   = key_stride;
	A.outStride   = out_stride;
	A.counts      = counts ? cp->dcounts.p : nullptr;
	A.rows        = cp->drows.p;
	A.curves      = cp->dcurves.p;
	A.state       = cp->state.p;
	A.meters      = d_meters;
	A.frames      = frames;
	A.nCurves     = cp->cfg.n_curves;
	A.nRows       = n;

	if (most == 0) { /* no frames: the launch only writes the meters, and is not a timed launch set */
		if (tbf_launch_comp (&A, s))
			return fail (-5, std::string ("k_comp launch failed: ") + hipGetErrorString (hipGetLastError ()));
		return 0;
	}
	StageTimer::Guard tg (cp->timer, s, "comp"); /* tbf_debug_comp_time: the launch between two events on its stream */
	if (int rc = tg.begin ())
		return rc;
	if (tbf_launch_comp (&A, s))
		return fail (-5, std::string ("k_comp launch failed: ") + hipGetErrorString (hipGetLastError ()));
	return tg.end ();
}

int tbf_comp_curve_design (double T, double R, double W, float* pts)
{
	if (!pts)
		return fail (-22, "comp: pts is NULL");
	if (!(T >= -90.0 && T <= 0.0))
		return fail (-22, "comp: threshold_db " + std::to_string (T) + " is not in [-90, 0]");
	if (!(R >= 1.0))
		return fail (-22, "comp: ratio " + std::to_string (R) + " is not in [1, +Inf]");
	if (!(W >= 0.0 && W <= 40.0))
		return fail (-22, "comp: knee_db " + std::to_string (W) + " is not in [0, 40]");
	const double slope = 1.0 / R; /* 0 at ratio +Inf */
	for (uint32_t i = 0; i < TBF_COMP_POINTS; i++) {
		const double level = std::ldexp (1.0 + (double)(i % TBF_COMP_SEG) / (double)TBF_COMP_SEG, (int)(i / TBF_COMP_SEG) - 16);
		const double x     = 20.0 * std::log10 (level);
		double       y;
		if (2.0 * (x - T) < -W)
			y = x;
		else if (2.0 * std::fabs (x - T) <= W) /* W > 0 here: with W == 0 only x == T arrives, below */
			y = W > 0.0 ? x + (slope - 1.0) * (x - T + W / 2.0) * (x - T + W / 2.0) / (2.0 * W) : x;
		else
			y = T + (x - T) * slope;
		pts[i] = (float)std::min (1.0, std::pow (10.0, (y - x) / 20.0));
	}
	return 0;
}

int tbf_debug_comp_ref (const float* pts, float attack, float release, float makeup, const float* L, const float* R, const float* keyL,
                        const float* keyR, uint64_t n, float* g, float* outL, float* outR, float* gains)
{
	if (!pts || !g)
		return fail (-22, std::string ("comp: ") + (pts ? "g" : "pts") + " is NULL");
	if (int rc = checkPoints (pts))
		return rc;
	if (int rc = checkRow (tbf_comp_row{0u, attack, release, makeup}, 0u, 0u))
		return rc;
	if (!(*g >= 0.0f && *g <= 1.0f))
		return fail (-22, "comp: g " + std::to_string (*g) + " is not in [0, 1]");
	if ((keyL == nullptr) != (keyR == nullptr))
		return fail (-22, "comp: one key plane is NULL and the other is not");
	if (n && (!L || !R || !outL || !outR))
		return fail (-22, "comp: a plane is NULL");
	const float* const kl = keyL ? keyL : L;
	const float* const kr = keyL ? keyR : R;
	float              gg = *g;
	for (uint64_t i = 0; i < n; i++) {
		const float t = comp_lookup (pts, limit_peak (kl[i], kr[i]));
		gg            = comp_step (gg, t, attack, release);
		if (gains)
			gains[i] = gg;
		outL[i] = comp_out (gg, makeup, L[i]);
		outR[i] = comp_out (gg, makeup, R[i]);
	}
	*g = gg;
	return 0;
}

int tbf_debug_comp_lookup (const float* pts, const float* levels, uint64_t n, float* t)
{
	if (!pts)
		return fail (-22, "comp: pts is NULL");
	if (int rc = checkPoints (pts))
		return rc;
	if (n && (!levels || !t))
		return fail (-22, std::string ("comp: ") + (levels ? "t" : "levels") + " is NULL");
	for (uint64_t i = 0; i < n; i++)
		if (!(levels[i] >= 0.0f))
			return fail (-22, "comp: level " + std::to_string (i) + " is negative or NaN");
	for (uint64_t i = 0; i < n; i++)
		t[i] = comp_lookup (pts, levels[i]);
	return 0;
}

int tbf_debug_comp_grid (uint32_t n_rows, uint32_t n_curves, uint32_t* rows_per_wave, uint32_t* tile_frames, uint32_t* lds_bytes)
{
	if (n_rows == 0)
		return fail (-22, "comp: n_rows is 0");
	if (int rc = checkCurves (n_curves))
		return rc;
	const uint32_t R = comp_rows (n_rows);
	if (rows_per_wave)
		*rows_per_wave = R;
	if (tile_frames)
		*tile_frames = TBF_COMP_TILE;
	if (lds_bytes)
		*lds_bytes = comp_lds_floats (R, n_curves) * 4u;
	return 0;
}

int tbf_debug_comp_time (tbf_comp* cp, int32_t enable, double* ms, uint64_t* launches)
{
	if (!cp)
		return fail (-22, "comp: comp is NULL");
	return cp->timer.query (enable, ms, launches);
}

} /* extern "C" */
