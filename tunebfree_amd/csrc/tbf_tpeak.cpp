/*
 * tbf_tpeak.cpp -- the host side of the true-peak meter: the meter objects an engine owns,
 * tbf_true_peak_device, reset, the read-out, and the tbf_debug_true_peak* hooks.
 *
 * A stage beside two float32 device planes (include/tbf.h): k_tpeak
 * (csrc/tbf_tpeak.hip) takes every row's two channels through the 4-phase interpolator of BS.1770-4
 * Annex 2 and keeps the largest magnitude of the samples and of the interpolated values as bit
 * patterns.  The state belongs to the meter, not to an instance: the render path, clone, save, load
 * and remove do not know it.  A row's history has two sides; a call reads the live one, writes the
 * other, and the host flips the side of every row that took frames, so the workgroups of a call
 * cannot race on it.  The host keeps every row's frame count.  tbf_debug_true_peak_ref is the
 * definition on the host, one row at a time, from tpeak_y and tpeak_mag of csrc/tbf_tpeak.h, which
 * the kernel runs.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_engine_impl.h"
#include "tbf_tpeak.h"

extern "C" int tbf_launch_tpeak (const tbf_tpeak_launch* P, hipStream_t stream);

using namespace tbf;

namespace {

int checkConfig (const tbf_true_peak_config* cfg)
{
	if (!cfg)
		return fail (-22, "true_peak: cfg is NULL");
	if (cfg->oversample != 1u && cfg->oversample != 2u && cfg->oversample != 4u)
		return fail (-22, "true_peak: oversample " + std::to_string (cfg->oversample) + " is none of 1, 2, 4");
	return 0;
}

float asFloat (uint32_t u)
{
	float f;
	memcpy (&f, &u, sizeof (f));
	return f;
}

/* 20 log10 of the largest of a row's four peaks: -HUGE_VAL for 0, NaN for a NaN (which the
 * unsigned maximum has put above everything) */
double tpeak_dbtp (const uint32_t* p4)
{
	const uint32_t m = std::max (std::max (p4[0], p4[1]), std::max (p4[2], p4[3]));
	if (m == 0u)
		return -HUGE_VAL;
	const float f = asFloat (m);
	return f != f ? (double)NAN : 20.0 * log10 ((double)f);
}

} // namespace

extern "C" {

int tbf_true_peak_create (tbf_engine* e, uint32_t n_rows, const tbf_true_peak_config* cfg, tbf_true_peak** out)
{
	if (!e)
		return fail (-22, "true_peak: engine is NULL");
	if (!out)
		return fail (-22, "true_peak: out is NULL");
	if (int rc = checkConfig (cfg))
		return rc;
	if (n_rows == 0)
		return fail (-22, "true_peak: n_rows is 0");
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) has no device to measure on");
	HIPCHK (hipSetDevice (e->cfg.device));
	std::unique_ptr<tbf_true_peak> tp (new tbf_true_peak ());
	tp->eng   = e;
	tp->cfg   = *cfg;
	tp->nRows = n_rows;
	const size_t floats = (size_t)n_rows * TBF_TPEAK_ROW_HIST, words = (size_t)n_rows * 4u;
	if (tp->hist.ensure (floats) || tp->peaks.ensure (words) || tp->drows.ensure (n_rows)) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (true-peak state: 200 B per row)");
	}
	HIPCHK (hipMemsetAsync (tp->hist.p, 0, floats * sizeof (float), e->stream));
	HIPCHK (hipMemsetAsync (tp->peaks.p, 0, words * sizeof (uint32_t), e->stream));
	HIPCHK (hipStreamSynchronize (e->stream));
	tp->rows.assign (n_rows, tbf_tpeak_row{0u, 0u});
	tp->pos.assign (n_rows, 0u);
	*out = tp.get ();
	e->truePeaks.push_back (std::move (tp));
	return 0;
}

int tbf_true_peak_destroy (tbf_true_peak* tp)
{
	if (!tp)
		return 0;
	auto it = slotOf (tp->eng->truePeaks, tp);
	if (it == tp->eng->truePeaks.end ())
		return fail (-22, "true_peak: not a meter of its engine");
	(void)hipSetDevice (tp->eng->cfg.device);
	tp->eng->truePeaks.erase (it); /* hipFree waits for the work that still writes the state */
	return 0;
}

int tbf_true_peak_reset (tbf_true_peak* tp, uint32_t n, const uint32_t* rows, void* stream)
{
	if (!tp)
		return fail (-22, "true_peak: tp is NULL");
	if (int rc = checkRows ("true_peak", n, rows, tp->nRows))
		return rc;
	HIPCHK (hipSetDevice (tp->eng->cfg.device));
	hipStream_t const s  = streamOr (stream, tp->eng->stream);
	const size_t      hb = TBF_TPEAK_ROW_HIST * sizeof (float), pb = 4u * sizeof (uint32_t); /* a row's history, both sides, and its peaks */
	if (!rows) {
		HIPCHK (hipMemsetAsync (tp->hist.p, 0, (size_t)tp->nRows * hb, s));
		HIPCHK (hipMemsetAsync (tp->peaks.p, 0, (size_t)tp->nRows * pb, s));
		std::fill (tp->pos.begin (), tp->pos.end (), 0u);
	}
	for (uint32_t k = 0; rows && k < n; k++) {
		HIPCHK (hipMemsetAsync (tp->hist.p + (size_t)rows[k] * TBF_TPEAK_ROW_HIST, 0, hb, s));
		HIPCHK (hipMemsetAsync (tp->peaks.p + (size_t)rows[k] * 4u, 0, pb, s));
		tp->pos[rows[k]] = 0u;
	}
	tp->last = s;
	return 0;
}

int tbf_true_peak_device (tbf_true_peak* tp, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames,
                          const uint32_t* counts, void* stream)
{
	if (!tp)
		return fail (-22, "true_peak: tp is NULL");
	if (!d_L || !d_R)
		return fail (-22, std::string ("true_peak: ") + (d_L ? "d_R" : "d_L") + " is NULL");
	if (in_stride < frames)
		return fail (-22, "true_peak: in_stride smaller than frames");
	if (((uintptr_t)d_L | (uintptr_t)d_R) & 3u)
		return fail (-22, "true_peak: device pointer not 4-byte aligned");
	const uint32_t n    = tp->nRows;
	uint32_t       most;
	if (int rc = countsMost ("true_peak", counts, n, frames, &most))
		return rc;
	const uint32_t tiles = (uint32_t)(((uint64_t)most + TBF_TPEAK_TILE - 1u) / TBF_TPEAK_TILE);
	if ((uint64_t)n * tiles > 0x7fffffffull)
		return fail (-22, "true_peak: frames " + std::to_string (most) + " of " + std::to_string (n) + " rows are more than one launch's 2^31 - 1 tiles");
	tbf_engine* const e = tp->eng;
	HIPCHK (hipSetDevice (e->cfg.device));
	hipStream_t const s = streamOr (stream, e->stream);
	if (most == 0)
		return 0;
	/* The rows on the device.  They are read from the meter's host vector, which the next call
	 * rewrites, so the stream is waited for. */
	for (uint32_t r = 0; r < n; r++)
		tp->rows[r].count = counts ? counts[r] : frames;
	HIPCHK (hipMemcpyAsync (tp->drows.p, tp->rows.data (), (size_t)n * sizeof (tbf_tpeak_row), hipMemcpyHostToDevice, s));
	HIPCHK (hipStreamSynchronize (s));

	tbf_tpeak_launch P;
	memset (&P, 0, sizeof (P));
	P.in[0]    = d_L;
	P.in[1]    = d_R;
	P.inStride = in_stride;
	P.rows     = tp->drows.p;
	P.hist     = tp->hist.p;
	P.peaks    = tp->peaks.p;
	P.nRows    = n;
	P.tiles    = tiles;
	P.F        = tp->cfg.oversample;

	StageTimer::Guard tg (tp->timer, s, "true_peak"); /* tbf_debug_true_peak_time: the launch between two events on its stream */
	if (int rc = tg.begin ())
		return rc;
	if (tbf_launch_tpeak (&P, s))
		return fail (-5, std::string ("k_tpeak launch failed: ") + hipGetErrorString (hipGetLastError ()));
	for (uint32_t r = 0; r < n; r++)
		if (tp->rows[r].count) { /* the launch wrote the other side of the rows that took frames */
			tp->rows[r].side ^= 1u;
			tp->pos[r] += tp->rows[r].count;
		}
	tp->last = s;
	return tg.end ();
}

int tbf_true_peak_read (tbf_true_peak* tp, uint32_t n, const uint32_t* rows, tbf_true_peak_result* out)
{
	if (!tp)
		return fail (-22, "true_peak: tp is NULL");
	if (!out)
		return fail (-22, "true_peak: out is NULL");
	if (!rows)
		n = tp->nRows;
	if (int rc = checkRows ("true_peak", n, rows, tp->nRows))
		return rc;
	HIPCHK (hipSetDevice (tp->eng->cfg.device));
	HIPCHK (hipStreamSynchronize (tp->last ? tp->last : tp->eng->stream));
	std::vector<uint32_t> w ((size_t)tp->nRows * 4u);
	HIPCHK (hipMemcpy (w.data (), tp->peaks.p, w.size () * sizeof (uint32_t), hipMemcpyDeviceToHost));
	for (uint32_t k = 0; k < n; k++) {
		const uint32_t  r = rows ? rows[k] : k;
		const uint32_t* p = w.data () + (size_t)r * 4u;
		out[k].sample_peak[0] = asFloat (p[0]);
		out[k].sample_peak[1] = asFloat (p[1]);
		out[k].inter_peak[0]  = asFloat (p[2]);
		out[k].inter_peak[1]  = asFloat (p[3]);
		out[k].frames         = tp->pos[r];
		out[k].dbtp           = tpeak_dbtp (p);
	}
	return 0;
}

int tbf_debug_true_peak_table (float* h48)
{
	if (!h48)
		return fail (-22, "true_peak: h48 is NULL");
	for (uint32_t p = 0; p < 4u; p++)
		for (uint32_t j = 0; j < TBF_TPEAK_TAPS; j++)
			h48[p * TBF_TPEAK_TAPS + j] = tpeak_h (p, j);
	return 0;
}

int tbf_debug_true_peak_ref (const tbf_true_peak_config* cfg, const float* L, const float* R, uint64_t n, float* hist22,
                             uint32_t* peaks4, float* y)
{
	if (int rc = checkConfig (cfg))
		return rc;
	if (!hist22)
		return fail (-22, "true_peak: hist22 is NULL");
	if (!peaks4)
		return fail (-22, "true_peak: peaks4 is NULL");
	if (n && (!L || !R))
		return fail (-22, std::string ("true_peak: ") + (L ? "R" : "L") + " is NULL");
	const uint32_t     F = cfg->oversample, np = tpeak_phases (F);
	std::vector<float> x ((size_t)TBF_TPEAK_HIST + n);
	for (uint32_t ch = 0; ch < 2u; ch++) {
		const float* in = ch ? R : L;
		float*       h  = hist22 + ch * TBF_TPEAK_HIST;
		std::copy (h, h + TBF_TPEAK_HIST, x.begin ());
		if (n)
			std::copy (in, in + n, x.begin () + TBF_TPEAK_HIST);
		uint32_t sp = peaks4[ch], ip = peaks4[2u + ch];
		for (uint64_t i = 0; i < n; i++) {
			const float* newest = x.data () + TBF_TPEAK_HIST + i;
			sp                  = std::max (sp, tpeak_mag (*newest));
			for (uint32_t q = 0; q < np; q++) {
				const float v = tpeak_y (tpeak_phase (F, q), newest);
				ip            = std::max (ip, tpeak_mag (v));
				if (y)
					y[((size_t)ch * n + i) * np + q] = v;
			}
		}
		peaks4[ch]      = sp;
		peaks4[2u + ch] = ip;
		std::copy (x.end () - TBF_TPEAK_HIST, x.end (), h); /* the last 11 of (history || frames) */
	}
	return 0;
}

int tbf_debug_true_peak_dbtp (const uint32_t* peaks4, double* dbtp)
{
	if (!peaks4 || !dbtp)
		return fail (-22, std::string ("true_peak: ") + (peaks4 ? "dbtp" : "peaks4") + " is NULL");
	*dbtp = tpeak_dbtp (peaks4);
	return 0;
}

int tbf_debug_true_peak_grid (uint32_t n_rows, uint32_t frames, uint32_t* tile_frames, uint32_t* frames_per_lane, uint64_t* groups,
                              uint32_t* lds_bytes)
{
	if (tile_frames)
		*tile_frames = TBF_TPEAK_TILE;
	if (frames_per_lane)
		*frames_per_lane = TBF_TPEAK_PER_LANE;
	if (groups)
		*groups = (uint64_t)n_rows * (((uint64_t)frames + TBF_TPEAK_TILE - 1u) / TBF_TPEAK_TILE);
	if (lds_bytes)
		*lds_bytes = TBF_TPEAK_LDS_BYTES;
	return 0;
}

int tbf_debug_true_peak_time (tbf_true_peak* tp, int32_t enable, double* ms, uint64_t* launches)
{
	if (!tp)
		return fail (-22, "true_peak: tp is NULL");
	return tp->timer.query (enable, ms, launches);
}

} /* extern "C" */
