/*
 * tbf_limit.cpp -- the host side of the bus limiter: the limiter objects an engine owns,
 * tbf_limit_device, reset, and the tbf_debug_limit* hooks.
 *
 * A post-stage on two float32 device planes (include/tbf.h): k_limit
 * (csrc/tbf_limit.hip) limits each row's peaks to a ceiling with look-ahead, hold and a linear
 * release.  The state, the last Hn input frames per row and channel, belongs to the limiter, not
 * to an instance: the render path, clone, save, load and remove do not know it.  A row keeps two
 * history buffers; a call reads the live one and writes the other, and the host flips the side of
 * every row that took frames once the launch is issued (tbf_limiter.rows), so no tile of a call
 * reads what another one writes.  Everything is checked before anything is staged or launched: a
 * refused call writes nothing and moves no state.  tbf_debug_limit_ref is the definition on the
 * host, one row at a time, from the functions of csrc/tbf_limit.h that the kernel runs.
 *
 * A limiter made by tbf_limiter_create_tp carries a true-peak detector (oversample 2 or 4): its
 * history is 11 frames longer, its latency 6, and its launch is k_limit_tp's
 * (csrc/tbf_limit_tp.hip).  Everything else, the argument checks included, is the one path below;
 * tbf_debug_limit_tp_ref differs from the plain restatement in its t alone.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_engine_impl.h"
#include "tbf_limit.h"

extern "C" int tbf_launch_limit (const tbf_limit_launch* P, hipStream_t stream);
extern "C" int tbf_launch_limit_tp (const tbf_limit_launch* P, uint32_t F, hipStream_t stream);

using namespace tbf;

namespace {

int checkConfig (const tbf_limiter_config* cfg)
{
	if (!cfg)
		return fail (-22, "limit: cfg is NULL");
	if (!std::isfinite (cfg->ceiling) || !(cfg->ceiling > 0.0f))
		return fail (-22, "limit: ceiling is not finite and positive");
	if (cfg->ahead < 2u || cfg->ahead > TBF_LIMIT_MAX_AHEAD || (cfg->ahead & (cfg->ahead - 1u)))
		return fail (-22, "limit: ahead " + std::to_string (cfg->ahead) + " is no power of two in [2, " +
		                      std::to_string (TBF_LIMIT_MAX_AHEAD) + "]");
	if (cfg->hold > TBF_LIMIT_MAX_HOLD)
		return fail (-22, "limit: hold " + std::to_string (cfg->hold) + " above " + std::to_string (TBF_LIMIT_MAX_HOLD));
	return 0;
}

int checkDetect (const tbf_limiter_detect* det)
{
	if (!det)
		return fail (-22, "limit: det is NULL");
	if (det->oversample != 2u && det->oversample != 4u)
		return fail (-22, "limit: oversample " + std::to_string (det->oversample) + " is none of 2, 4");
	if (det->reserved != 0u)
		return fail (-22, "limit: det->reserved is not 0");
	return 0;
}

/* a limiter of either kind: det NULL for the plain one */
int createLimiter (tbf_engine* e, uint32_t n_rows, const tbf_limiter_config* cfg, const tbf_limiter_detect* det, bool tp,
                   tbf_limiter** out)
{
	if (!e)
		return fail (-22, "limit: engine is NULL");
	if (!out)
		return fail (-22, "limit: out is NULL");
	if (int rc = checkConfig (cfg))
		return rc;
	if (tp)
		if (int rc = checkDetect (det))
			return rc;
	if (n_rows == 0)
		return fail (-22, "limit: n_rows is 0");
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) has no device to limit on");
	HIPCHK (hipSetDevice (e->cfg.device));
	std::unique_ptr<tbf_limiter> lim (new tbf_limiter ());
	lim->eng   = e;
	lim->cfg   = *cfg;
	lim->nRows = n_rows;
	lim->oversample = tp ? det->oversample : 0u;
	lim->Hn    = tp ? limit_tp_history (cfg->ahead, cfg->hold) : limit_history (cfg->ahead, cfg->hold);
	const size_t floats = (size_t)n_rows * 4u * lim->Hn;
	if (lim->hist.ensure (floats) || lim->drows.ensure (n_rows)) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (limiter state: 16 B per row and frame of history)");
	}
	HIPCHK (hipMemsetAsync (lim->hist.p, 0, floats * sizeof (float), e->stream));
	HIPCHK (hipStreamSynchronize (e->stream));
	lim->rows.assign (n_rows, tbf_limit_row{0u, 0u});
	*out = lim.get ();
	e->limiters.push_back (std::move (lim));
	return 0;
}

/* What both host restatements share behind their t: x = the row's history of hn frames and the
 * call's n frames as one row (frame i of it being frame i - hn of the call), t per frame of it from
 * index hn - (2 A + H - 2) on (what lies before is never read), the output `delay` frames late. */
void gainAndOut (const tbf_limiter_config* cfg, uint32_t hn, uint32_t delay, const std::vector<float>& xl,
                 const std::vector<float>& xr, const std::vector<float>& t, uint64_t n, float* outL, float* outR,
                 tbf_limit_meter* meter)
{
	const float    c = cfg->ceiling;
	const uint32_t A = cfg->ahead, W = A + cfg->hold;
	const uint64_t N = (uint64_t)hn + n;
	std::vector<float> m (N);
	/* m[i] = min t[i - W + 1 .. i] (what lies before the row's start is never used): the indices
	 * of a non-decreasing run of candidates, the front one the window's minimum */
	{
		std::vector<uint64_t> q (N);
		uint64_t              head = 0, tail = 0;
		for (uint64_t i = 0; i < N; i++) {
			while (tail > head && !(t[q[tail - 1]] < t[i]))
				tail--;
			q[tail++] = i;
			if (q[head] + W <= i)
				head++;
			m[i] = t[q[head]];
		}
	}
	const float inv = 1.0f / (float)A;
	float       minG = 1.0f;
	uint32_t    reduced = 0, clamped = 0;
	for (uint64_t j = 0; j < n; j++) {
		const uint64_t i   = hn + j;
		float          acc = 0.0f;
		for (uint64_t k = i - A + 1u; k <= i; k++)
			acc = acc + m[k];
		const float g = acc * inv;
		outL[j]       = limit_out (g, xl[i - delay], c, clamped);
		outR[j]       = limit_out (g, xr[i - delay], c, clamped);
		if (g < minG)
			minG = g;
		reduced += g < 1.0f ? 1u : 0u;
	}
	if (meter)
		*meter = {minG, reduced, clamped};
}

} // namespace

extern "C" {

int tbf_limiter_create (tbf_engine* e, uint32_t n_rows, const tbf_limiter_config* cfg, tbf_limiter** out)
{
	return createLimiter (e, n_rows, cfg, nullptr, false, out);
}

int tbf_limiter_create_tp (tbf_engine* e, uint32_t n_rows, const tbf_limiter_config* cfg, const tbf_limiter_detect* det,
                           tbf_limiter** out)
{
	return createLimiter (e, n_rows, cfg, det, true, out);
}

int tbf_limiter_destroy (tbf_limiter* lim)
{
	if (!lim)
		return 0;
	auto it = slotOf (lim->eng->limiters, lim);
	if (it == lim->eng->limiters.end ())
		return fail (-22, "limit: not a limiter of its engine");
	(void)hipSetDevice (lim->eng->cfg.device);
	lim->eng->limiters.erase (it); /* hipFree waits for the work that still reads the state */
	return 0;
}

int tbf_limiter_reset (tbf_limiter* lim, uint32_t n, const uint32_t* rows, void* stream)
{
	if (!lim)
		return fail (-22, "limit: lim is NULL");
	if (int rc = checkRows ("limit", n, rows, lim->nRows))
		return rc;
	HIPCHK (hipSetDevice (lim->eng->cfg.device));
	hipStream_t const s = streamOr (stream, lim->eng->stream);
	const size_t      per = (size_t)4u * lim->Hn; /* a row's floats: both sides, both channels */
	if (!rows)
		HIPCHK (hipMemsetAsync (lim->hist.p, 0, (size_t)lim->nRows * per * sizeof (float), s));
	for (uint32_t k = 0; rows && k < n; k++)
		HIPCHK (hipMemsetAsync (lim->hist.p + (size_t)rows[k] * per, 0, per * sizeof (float), s));
	return 0;
}

int tbf_limiter_latency (const tbf_limiter* lim, uint32_t* frames)
{
	if (!lim)
		return fail (-22, "limit: lim is NULL");
	if (!frames)
		return fail (-22, "limit: frames is NULL");
	*frames = lim->cfg.ahead - 1u + (lim->oversample ? TBF_LIMIT_TP_DELAY : 0u);
	return 0;
}

int tbf_limit_device (tbf_limiter* lim, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames,
                      const uint32_t* counts, const tbf_limit_out* out, void* stream)
{
	if (!lim)
		return fail (-22, "limit: lim is NULL");
	if (!d_L || !d_R)
		return fail (-22, std::string ("limit: ") + (d_L ? "d_R" : "d_L") + " is NULL");
	if (!out)
		return fail (-22, "limit: out is NULL");
	if (!out->L || !out->R)
		return fail (-22, std::string ("limit: ") + (out->L ? "out->R" : "out->L") + " is NULL");
	if (in_stride < frames)
		return fail (-22, "limit: in_stride smaller than frames");
	if (out->stride < frames)
		return fail (-22, "limit: out stride smaller than frames");
	if (((uintptr_t)d_L | (uintptr_t)d_R | (uintptr_t)out->L | (uintptr_t)out->R | (uintptr_t)out->meters) & 3u)
		return fail (-22, "limit: device pointer not 4-byte aligned");
	const uint32_t n = lim->nRows;
	uint32_t       most;
	if (int rc = countsMost ("limit", counts, n, frames, &most))
		return rc;
	{
		const uint64_t rowBytes = (uint64_t)frames * 4;
		const Span     sp[5]    = {rowsSpan (d_L, n, in_stride * 4, rowBytes), rowsSpan (d_R, n, in_stride * 4, rowBytes),
		                           rowsSpan (out->L, n, out->stride * 4, rowBytes), rowsSpan (out->R, n, out->stride * 4, rowBytes),
		                           rowsSpan (out->meters, n, sizeof (tbf_limit_meter), sizeof (tbf_limit_meter))};
		if (anyOverlap (sp, 5, 2)) /* d_L and d_R may be one plane: mono */
			return fail (-22, "limit: input rows, output planes and meters overlap (in-place use is refused)");
	}
	tbf_engine* const e = lim->eng;
	HIPCHK (hipSetDevice (e->cfg.device));
	hipStream_t const s = streamOr (stream, e->stream);
	if (most == 0 && !out->meters)
		return 0;
	/* The rows' counts and sides on the device.  They are read from the limiter's host vector,
	 * which the next call rewrites, so the stream is waited for. */
	for (uint32_t r = 0; r < n; r++)
		lim->rows[r].count = counts ? counts[r] : frames;
	HIPCHK (hipMemcpyAsync (lim->drows.p, lim->rows.data (), (size_t)n * sizeof (tbf_limit_row), hipMemcpyHostToDevice, s));
	HIPCHK (hipStreamSynchronize (s));

	tbf_limit_launch P;
	memset (&P, 0, sizeof (P));
	P.in[0]     = d_L;
	P.in[1]     = d_R;
	P.inStride  = in_stride;
	P.out[0]    = out->L;
	P.out[1]    = out->R;
	P.outStride = out->stride;
	P.hist      = lim->hist.p;
	P.rows      = lim->drows.p;
	P.meters    = out->meters;
	P.ceiling   = lim->cfg.ceiling;
	P.ahead     = lim->cfg.ahead;
	P.hold      = lim->cfg.hold;
	P.maxCount  = most;

	StageTimer::Guard tg (lim->timer, s, "limit"); /* tbf_debug_limit_time: the launch set between two events on its stream */
	if (int rc = tg.begin ())
		return rc;
	for (uint32_t r0 = 0; r0 < n; r0 += TBF_LIMIT_MAX_ROWS) {
		P.rowBase = r0;
		P.nRows   = std::min (TBF_LIMIT_MAX_ROWS, n - r0);
		if (lim->oversample ? tbf_launch_limit_tp (&P, lim->oversample, s) : tbf_launch_limit (&P, s))
			return fail (-5, std::string (lim->oversample ? "k_limit_tp" : "k_limit") + " launch failed: " +
			                     hipGetErrorString (hipGetLastError ()));
	}
	for (uint32_t r = 0; r < n; r++) /* the rows that took frames now live on their other side */
		if (lim->rows[r].count)
			lim->rows[r].side ^= 1u;
	if (int rc = tg.end ())
		return rc;
	lim->launches++;
	return 0;
}

int tbf_debug_limit_ref (const tbf_limiter_config* cfg, const float* L, const float* R, uint64_t n, float* histL, float* histR,
                         float* outL, float* outR, tbf_limit_meter* meter)
{
	if (int rc = checkConfig (cfg))
		return rc;
	if (!histL || !histR)
		return fail (-22, std::string ("limit: ") + (histL ? "histR" : "histL") + " is NULL");
	if (n && (!L || !R || !outL || !outR))
		return fail (-22, "limit: a plane is NULL");
	const float    c = cfg->ceiling;
	const uint32_t A = cfg->ahead, D = A - 1u, Hn = limit_history (A, cfg->hold);
	const uint64_t N = (uint64_t)Hn + n;
	/* the history and the call's frames as one row, frame i of it being frame i - Hn of the call */
	std::vector<float> xl (N), xr (N), t (N);
	memcpy (xl.data (), histL, (size_t)Hn * 4), memcpy (xr.data (), histR, (size_t)Hn * 4);
	if (n)
		memcpy (xl.data () + Hn, L, (size_t)n * 4), memcpy (xr.data () + Hn, R, (size_t)n * 4);
	for (uint64_t i = 0; i < N; i++)
		t[i] = limit_target (limit_peak (xl[i], xr[i]), c);
	gainAndOut (cfg, Hn, D, xl, xr, t, n, outL, outR, meter);
	memcpy (histL, xl.data () + n, (size_t)Hn * 4), memcpy (histR, xr.data () + n, (size_t)Hn * 4);
	return 0;
}

int tbf_debug_limit_tp_ref (const tbf_limiter_config* cfg, const tbf_limiter_detect* det, const float* L, const float* R, uint64_t n,
                            float* histL, float* histR, float* outL, float* outR, tbf_limit_meter* meter)
{
	if (int rc = checkConfig (cfg))
		return rc;
	if (int rc = checkDetect (det))
		return rc;
	if (!histL || !histR)
		return fail (-22, std::string ("limit: ") + (histL ? "histR" : "histL") + " is NULL");
	if (n && (!L || !R || !outL || !outR))
		return fail (-22, "limit: a plane is NULL");
	const uint32_t Ht = limit_tp_history (cfg->ahead, cfg->hold), DE = cfg->ahead - 1u + TBF_LIMIT_TP_DELAY;
	const uint64_t N  = (uint64_t)Ht + n;
	/* the history and the call's frames as one row, frame i of it being frame i - Hn_tp of the call */
	std::vector<float> xl (N), xr (N), t (N);
	memcpy (xl.data (), histL, (size_t)Ht * 4), memcpy (xr.data (), histR, (size_t)Ht * 4);
	if (n)
		memcpy (xl.data () + Ht, L, (size_t)n * 4), memcpy (xr.data () + Ht, R, (size_t)n * 4);
	for (uint64_t i = 0; i < N; i++) /* the first 11 have no full window and are never read: g[n] reaches t[n - Hn] */
		t[i] = i < TBF_LIMIT_TP_REACH ? 1.0f : limit_target (limit_tp_peak (det->oversample, &xl[i], &xr[i]), cfg->ceiling);
	gainAndOut (cfg, Ht, DE, xl, xr, t, n, outL, outR, meter);
	memcpy (histL, xl.data () + n, (size_t)Ht * 4), memcpy (histR, xr.data () + n, (size_t)Ht * 4);
	return 0;
}

int tbf_debug_limit_grid (const tbf_limiter_config* cfg, uint32_t* frames_per_lane, uint32_t* tile_frames, uint32_t* history,
                          uint32_t* lds_bytes)
{
	if (int rc = checkConfig (cfg))
		return rc;
	if (frames_per_lane)
		*frames_per_lane = TBF_LIMIT_GROUP;
	if (tile_frames)
		*tile_frames = limit_tile (cfg->ahead, cfg->hold);
	if (history)
		*history = limit_history (cfg->ahead, cfg->hold);
	if (lds_bytes)
		*lds_bytes = 2u * limit_lds_floats (cfg->ahead, cfg->hold) * (uint32_t)sizeof (float);
	return 0;
}

int tbf_debug_limit_tp_grid (const tbf_limiter_config* cfg, const tbf_limiter_detect* det, uint32_t* frames_per_lane,
                             uint32_t* tile_frames, uint32_t* history, uint32_t* lds_bytes)
{
	if (int rc = checkConfig (cfg))
		return rc;
	if (int rc = checkDetect (det))
		return rc;
	if (frames_per_lane)
		*frames_per_lane = TBF_LIMIT_GROUP;
	if (tile_frames)
		*tile_frames = limit_tile (cfg->ahead, cfg->hold);
	if (history)
		*history = limit_tp_history (cfg->ahead, cfg->hold);
	if (lds_bytes)
		*lds_bytes = limit_tp_lds_bytes (cfg->ahead, cfg->hold);
	return 0;
}

int tbf_debug_limit_time (tbf_limiter* lim, int32_t enable, double* ms, uint64_t* launches)
{
	if (!lim)
		return fail (-22, "limit: lim is NULL");
	return lim->timer.query (enable, ms, launches);
}

} /* extern "C" */
