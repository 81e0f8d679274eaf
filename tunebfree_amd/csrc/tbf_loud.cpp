/*
 * tbf_loud.cpp -- the host side of the loudness meter: the meter objects an engine owns,
 * tbf_loudness_device, reset, the read-outs, the gating, and the tbf_debug_loudness* hooks.
 *
 * A stage beside two float32 device planes (include/tbf.h): k_loud
 * (csrc/tbf_loud.hip) runs every row's two channels through the K-weighting biquads in double and
 * writes the sum of squares of every complete 100 ms hop.  The state belongs to the meter, not to
 * an instance: the render path, clone, save, load and remove do not know it.  The host keeps every
 * row's position, so a call that would complete more hops than a row can hold is refused before
 * anything moves, and a read-out knows how many hops to fetch.  The loudness figures are the
 * gating of BS.1770-4 / EBU R128 over those energies, on the host in double (loud_result).
 * tbf_debug_loudness_ref is the definition on the host, one row at a time, from loud_step of
 * csrc/tbf_loud.h, which the kernel runs.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_engine_impl.h"
#include "tbf_loud.h"

extern "C" int tbf_launch_loud (const tbf_loud_launch* P, hipStream_t stream);

using namespace tbf;

namespace {

int checkRate (uint32_t rate)
{
	if (rate < TBF_LOUD_MIN_RATE || rate > TBF_LOUD_MAX_RATE || rate % 10u)
		return fail (-22, "loudness: rate_hz " + std::to_string (rate) + " is no multiple of 10 in [" +
		                      std::to_string (TBF_LOUD_MIN_RATE) + ", " + std::to_string (TBF_LOUD_MAX_RATE) + "]");
	return 0;
}

int checkConfig (const tbf_loudness_config* cfg)
{
	if (!cfg)
		return fail (-22, "loudness: cfg is NULL");
	if (int rc = checkRate (cfg->rate_hz))
		return rc;
	if (cfg->max_hops == 0)
		return fail (-22, "loudness: max_hops is 0");
	return 0;
}

/* b0, b1, b2, a1, a2 of the shelf and c1, c2 of the high-pass, as include/tbf.h spells them */
void coeffs (uint32_t rate, double* c)
{
	const double pi = 3.141592653589793;
	{
		const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
		const double K  = tan (pi * f0 / (double)rate);
		const double Vh = pow (10.0, G / 20.0), Vb = pow (Vh, 0.4996667741545416);
		const double a0 = 1.0 + K / Q + K * K;
		c[0]            = (Vh + Vb * K / Q + K * K) / a0;
		c[1]            = 2.0 * (K * K - Vh) / a0;
		c[2]            = (Vh - Vb * K / Q + K * K) / a0;
		c[3]            = 2.0 * (K * K - 1.0) / a0;
		c[4]            = (1.0 - K / Q + K * K) / a0;
	}
	{
		const double f0 = 38.13547087602444, Q = 0.5003270373238773;
		const double K  = tan (pi * f0 / (double)rate);
		const double a0 = 1.0 + K / Q + K * K;
		c[5]            = 2.0 * (K * K - 1.0) / a0;
		c[6]            = (1.0 - K / Q + K * K) / a0;
	}
}

double lufs (double z) { return -0.691 + 10.0 * log10 (z); }

/* the gating over n EL, ER pairs */
void loud_result (uint32_t rate, const double* e, uint32_t n, tbf_loudness_result* out)
{
	const double Hp = (double)(rate / 10u);
	out->integrated = out->momentary_max = out->short_term_max = -HUGE_VAL;
	out->hops                                                  = n;
	out->blocks = out->gated = out->reserved = 0u;
	if (n < 4u)
		return;
	const uint32_t      nb = n - 3u;
	std::vector<double> u (n), z (nb), l (nb);
	for (uint32_t h = 0; h < n; h++)
		u[h] = e[2u * h] + e[2u * h + 1u];
	out->blocks = nb;
	double sumAbs = 0.0;
	uint32_t nAbs = 0;
	for (uint32_t j = 0; j < nb; j++) {
		z[j] = (((u[j] + u[j + 1u]) + u[j + 2u]) + u[j + 3u]) / (4.0 * Hp);
		l[j] = lufs (z[j]);
		if (l[j] > out->momentary_max)
			out->momentary_max = l[j];
		if (l[j] > -70.0) {
			sumAbs = sumAbs + z[j];
			nAbs++;
		}
	}
	if (nAbs) {
		const double gate = lufs (sumAbs / (double)nAbs) - 10.0;
		double       sum  = 0.0;
		uint32_t     cnt  = 0;
		for (uint32_t j = 0; j < nb; j++)
			if (l[j] > -70.0 && l[j] > gate) {
				sum = sum + z[j];
				cnt++;
			}
		out->gated = cnt;
		if (cnt)
			out->integrated = lufs (sum / (double)cnt);
	}
	for (uint32_t j = 0; j + 30u <= n; j++) {
		double s = u[j];
		for (uint32_t i = 1; i < 30u; i++)
			s = s + u[j + i];
		const double ls = lufs (s / (30.0 * Hp));
		if (ls > out->short_term_max)
			out->short_term_max = ls;
	}
}

/* the loudness range of EBU Tech 3342 over n EL, ER pairs (include/tbf.h) */
void loud_range (uint32_t rate, const double* e, uint32_t n, double* lra, uint32_t* windows)
{
	const double Hp = (double)(rate / 10u);
	*lra            = 0.0;
	if (windows)
		*windows = 0u;
	if (n < 30u)
		return;
	const uint32_t      nw = n - 29u;
	std::vector<double> u (n), z (nw), l (nw);
	for (uint32_t h = 0; h < n; h++)
		u[h] = e[2u * h] + e[2u * h + 1u];
	double   sumAbs = 0.0;
	uint32_t nAbs   = 0;
	for (uint32_t j = 0; j < nw; j++) {
		double s = u[j];
		for (uint32_t i = 1; i < 30u; i++)
			s = s + u[j + i];
		z[j] = s / (30.0 * Hp);
		l[j] = lufs (z[j]);
		if (l[j] > -70.0) {
			sumAbs = sumAbs + z[j];
			nAbs++;
		}
	}
	if (!nAbs)
		return;
	const double        gate = lufs (sumAbs / (double)nAbs) - 20.0;
	std::vector<double> s;
	for (uint32_t j = 0; j < nw; j++)
		if (l[j] > -70.0 && l[j] > gate)
			s.push_back (l[j]);
	if (s.empty ())
		return;
	std::sort (s.begin (), s.end ());
	const double m = (double)(s.size () - 1u);
	*lra           = s[(size_t)floor (m * 0.95 + 0.5)] - s[(size_t)floor (m * 0.10 + 0.5)];
	if (windows)
		*windows = (uint32_t)s.size ();
}

/* the meter's last call has passed its stream */
int settle (tbf_loudness* lm)
{
	HIPCHK (hipSetDevice (lm->eng->cfg.device));
	HIPCHK (hipStreamSynchronize (lm->last ? lm->last : lm->eng->stream));
	return 0;
}

/* a row's first n hops from the device */
int fetch (tbf_loudness* lm, uint32_t row, uint32_t n, double* e)
{
	if (n)
		HIPCHK (hipMemcpy (e, lm->energy.p + (size_t)row * lm->cfg.max_hops * 2u, (size_t)n * 2u * sizeof (double), hipMemcpyDeviceToHost));
	return 0;
}

} // namespace

extern "C" {

int tbf_loudness_create (tbf_engine* e, uint32_t n_rows, const tbf_loudness_config* cfg, tbf_loudness** out)
{
	if (!e)
		return fail (-22, "loudness: engine is NULL");
	if (!out)
		return fail (-22, "loudness: out is NULL");
	if (int rc = checkConfig (cfg))
		return rc;
	if (n_rows == 0)
		return fail (-22, "loudness: n_rows is 0");
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) has no device to measure on");
	HIPCHK (hipSetDevice (e->cfg.device));
	std::unique_ptr<tbf_loudness> lm (new tbf_loudness ());
	lm->eng   = e;
	lm->cfg   = *cfg;
	lm->nRows = n_rows;
	lm->Hp    = cfg->rate_hz / 10u;
	coeffs (cfg->rate_hz, lm->c);
	const size_t chans = (size_t)n_rows * 2u, doubles = chans * cfg->max_hops;
	if (lm->state.ensure (chans) || lm->energy.ensure (doubles) || lm->dcounts.ensure (n_rows)) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (loudness state: 16 B per row and hop, and 96 B per row)");
	}
	HIPCHK (hipMemsetAsync (lm->state.p, 0, chans * sizeof (tbf_loud_chan), e->stream));
	HIPCHK (hipMemsetAsync (lm->energy.p, 0, doubles * sizeof (double), e->stream));
	HIPCHK (hipStreamSynchronize (e->stream));
	lm->counts.assign (n_rows, 0u);
	lm->pos.assign (n_rows, 0u);
	*out = lm.get ();
	e->loudness.push_back (std::move (lm));
	return 0;
}

int tbf_loudness_destroy (tbf_loudness* lm)
{
	if (!lm)
		return 0;
	auto it = slotOf (lm->eng->loudness, lm);
	if (it == lm->eng->loudness.end ())
		return fail (-22, "loudness: not a meter of its engine");
	(void)hipSetDevice (lm->eng->cfg.device);
	lm->eng->loudness.erase (it); /* hipFree waits for the work that still writes the state */
	return 0;
}

int tbf_loudness_reset (tbf_loudness* lm, uint32_t n, const uint32_t* rows, void* stream)
{
	if (!lm)
		return fail (-22, "loudness: lm is NULL");
	if (int rc = checkRows ("loudness", n, rows, lm->nRows))
		return rc;
	HIPCHK (hipSetDevice (lm->eng->cfg.device));
	hipStream_t const s   = streamOr (stream, lm->eng->stream);
	const size_t      per = 2u * sizeof (tbf_loud_chan); /* a row's state: both channels */
	if (!rows) {
		HIPCHK (hipMemsetAsync (lm->state.p, 0, (size_t)lm->nRows * per, s));
		std::fill (lm->pos.begin (), lm->pos.end (), 0u);
	}
	for (uint32_t k = 0; rows && k < n; k++) {
		HIPCHK (hipMemsetAsync (lm->state.p + (size_t)rows[k] * 2u, 0, per, s));
		lm->pos[rows[k]] = 0u;
	}
	lm->last = s;
	return 0;
}

int tbf_loudness_device (tbf_loudness* lm, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames,
                         const uint32_t* counts, void* stream)
{
	if (!lm)
		return fail (-22, "loudness: lm is NULL");
	if (!d_L || !d_R)
		return fail (-22, std::string ("loudness: ") + (d_L ? "d_R" : "d_L") + " is NULL");
	if (in_stride < frames)
		return fail (-22, "loudness: in_stride smaller than frames");
	if (((uintptr_t)d_L | (uintptr_t)d_R) & 3u)
		return fail (-22, "loudness: device pointer not 4-byte aligned");
	const uint32_t n    = lm->nRows;
	uint32_t       most;
	if (int rc = countsMost ("loudness", counts, n, frames, &most))
		return rc;
	for (uint32_t r = 0; r < n; r++) {
		const uint64_t c = counts ? counts[r] : frames;
		if ((lm->pos[r] + c) / lm->Hp > lm->cfg.max_hops)
			return fail (-28, "loudness: row " + std::to_string (r) + " would complete " + std::to_string ((lm->pos[r] + c) / lm->Hp) +
			                      " hops, max_hops is " + std::to_string (lm->cfg.max_hops));
	}
	tbf_engine* const e = lm->eng;
	HIPCHK (hipSetDevice (e->cfg.device));
	hipStream_t const s = streamOr (stream, e->stream);
	if (most == 0)
		return 0;
	/* The counts on the device.  They are read from the meter's host vector, which the next call
	 * rewrites, so the stream is waited for. */
	for (uint32_t r = 0; r < n; r++)
		lm->counts[r] = counts ? counts[r] : frames;
	HIPCHK (hipMemcpyAsync (lm->dcounts.p, lm->counts.data (), (size_t)n * sizeof (uint32_t), hipMemcpyHostToDevice, s));
	HIPCHK (hipStreamSynchronize (s));

	tbf_loud_launch P;
	memset (&P, 0, sizeof (P));
	P.in[0]    = d_L;
	P.in[1]    = d_R;
	P.inStride = in_stride;
	P.counts   = lm->dcounts.p;
	P.state    = lm->state.p;
	P.energy   = lm->energy.p;
	memcpy (P.c, lm->c, sizeof (P.c));
	P.Hp      = lm->Hp;
	P.maxHops = lm->cfg.max_hops;
	P.nRows   = n;

	StageTimer::Guard tg (lm->timer, s, "loudness"); /* tbf_debug_loudness_time: the launch between two events on its stream */
	if (int rc = tg.begin ())
		return rc;
	if (tbf_launch_loud (&P, s))
		return fail (-5, std::string ("k_loud launch failed: ") + hipGetErrorString (hipGetLastError ()));
	for (uint32_t r = 0; r < n; r++)
		lm->pos[r] += lm->counts[r];
	lm->last = s;
	return tg.end ();
}

int tbf_loudness_read (tbf_loudness* lm, uint32_t n, const uint32_t* rows, tbf_loudness_result* out)
{
	if (!lm)
		return fail (-22, "loudness: lm is NULL");
	if (!out)
		return fail (-22, "loudness: out is NULL");
	if (!rows)
		n = lm->nRows;
	if (int rc = checkRows ("loudness", n, rows, lm->nRows))
		return rc;
	if (int rc = settle (lm))
		return rc;
	std::vector<double> e;
	for (uint32_t k = 0; k < n; k++) {
		const uint32_t r = rows ? rows[k] : k;
		const uint32_t N = (uint32_t)(lm->pos[r] / lm->Hp);
		e.resize ((size_t)N * 2u);
		if (int rc = fetch (lm, r, N, e.data ()))
			return rc;
		loud_result (lm->cfg.rate_hz, e.data (), N, out + k);
	}
	return 0;
}

int tbf_loudness_hops (tbf_loudness* lm, uint32_t row, double* e, uint32_t cap_hops, uint32_t* n_hops)
{
	if (!lm)
		return fail (-22, "loudness: lm is NULL");
	if (!n_hops)
		return fail (-22, "loudness: n_hops is NULL");
	if (row >= lm->nRows)
		return fail (-22, "loudness: row " + std::to_string (row) + " is no row of n_rows " + std::to_string (lm->nRows));
	const uint32_t N = (uint32_t)(lm->pos[row] / lm->Hp);
	*n_hops          = N;
	if (N > cap_hops)
		return fail (-28, "loudness: " + std::to_string (N) + " hops, cap_hops is " + std::to_string (cap_hops));
	if (N && !e)
		return fail (-22, "loudness: e is NULL");
	if (int rc = settle (lm))
		return rc;
	return fetch (lm, row, N, e);
}

int tbf_debug_loudness_coeffs (uint32_t rate_hz, double* c7)
{
	if (int rc = checkRate (rate_hz))
		return rc;
	if (!c7)
		return fail (-22, "loudness: c7 is NULL");
	coeffs (rate_hz, c7);
	return 0;
}

int tbf_debug_loudness_ref (const tbf_loudness_config* cfg, const float* L, const float* R, uint64_t n, double* state,
                            double* e, uint32_t cap_hops, uint32_t* n_hops)
{
	if (int rc = checkConfig (cfg))
		return rc;
	if (!state)
		return fail (-22, "loudness: state is NULL");
	if (!n_hops)
		return fail (-22, "loudness: n_hops is NULL");
	if (n && (!L || !R))
		return fail (-22, std::string ("loudness: ") + (L ? "R" : "L") + " is NULL");
	const uint32_t Hp = cfg->rate_hz / 10u;
	tbf_loud_chan  S[2];
	uint64_t       need = 0;
	for (int ch = 0; ch < 2; ch++) {
		const double* st = state + 6 * ch;
		if (!(st[5] >= 0.0 && st[5] < (double)Hp && st[5] == floor (st[5])))
			return fail (-22, "loudness: state k is no integer in [0, Hp)");
		S[ch] = {st[0], st[1], st[2], st[3], st[4], (uint32_t)st[5], 0u};
		need  = std::max (need, ((uint64_t)S[ch].k + n) / Hp);
	}
	if (need > cap_hops)
		return fail (-28, "loudness: " + std::to_string (need) + " hops, cap_hops is " + std::to_string (cap_hops));
	if (need && !e)
		return fail (-22, "loudness: e is NULL");
	double c[7];
	coeffs (cfg->rate_hz, c);
	for (int ch = 0; ch < 2; ch++) {
		const float* x = ch ? R : L;
		for (uint64_t i = 0; i < n; i++) {
			loud_step (c, (double)x[i], S[ch]);
			if (S[ch].k == Hp) {
				e[(size_t)S[ch].hop * 2u + ch] = S[ch].acc;
				S[ch].acc                      = 0.0;
				S[ch].k                        = 0u;
				S[ch].hop++;
			}
		}
		double* st = state + 6 * ch;
		st[0] = S[ch].s1, st[1] = S[ch].s2, st[2] = S[ch].t1, st[3] = S[ch].t2, st[4] = S[ch].acc, st[5] = (double)S[ch].k;
	}
	*n_hops = (uint32_t)need;
	return 0;
}

int tbf_debug_loudness_result (uint32_t rate_hz, const double* e, uint32_t n_hops, tbf_loudness_result* out)
{
	if (int rc = checkRate (rate_hz))
		return rc;
	if (!out)
		return fail (-22, "loudness: out is NULL");
	if (n_hops && !e)
		return fail (-22, "loudness: e is NULL");
	loud_result (rate_hz, e, n_hops, out);
	return 0;
}

int tbf_loudness_range (tbf_loudness* lm, uint32_t n, const uint32_t* rows, double* lra, uint32_t* windows)
{
	if (!lm)
		return fail (-22, "loudness: lm is NULL");
	if (!lra)
		return fail (-22, "loudness: lra is NULL");
	if (!rows)
		n = lm->nRows;
	if (int rc = checkRows ("loudness", n, rows, lm->nRows))
		return rc;
	if (int rc = settle (lm))
		return rc;
	std::vector<double> e;
	for (uint32_t k = 0; k < n; k++) {
		const uint32_t r = rows ? rows[k] : k;
		const uint32_t N = (uint32_t)(lm->pos[r] / lm->Hp);
		e.resize ((size_t)N * 2u);
		if (int rc = fetch (lm, r, N, e.data ()))
			return rc;
		loud_range (lm->cfg.rate_hz, e.data (), N, lra + k, windows ? windows + k : nullptr);
	}
	return 0;
}

int tbf_debug_loudness_range (uint32_t rate_hz, const double* e, uint32_t n_hops, double* lra, uint32_t* windows)
{
	if (int rc = checkRate (rate_hz))
		return rc;
	if (!lra)
		return fail (-22, "loudness: lra is NULL");
	if (n_hops && !e)
		return fail (-22, "loudness: e is NULL");
	loud_range (rate_hz, e, n_hops, lra, windows);
	return 0;
}

int tbf_debug_loudness_grid (uint32_t n_rows, uint32_t* rows_per_group, uint32_t* tile_frames, uint32_t* lds_bytes)
{
	(void)n_rows; /* one layout for every meter */
	if (rows_per_group)
		*rows_per_group = TBF_LOUD_ROWS;
	if (tile_frames)
		*tile_frames = TBF_LOUD_TILE;
	if (lds_bytes)
		*lds_bytes = TBF_LOUD_LDS_BYTES;
	return 0;
}

int tbf_debug_loudness_time (tbf_loudness* lm, int32_t enable, double* ms, uint64_t* launches)
{
	if (!lm)
		return fail (-22, "loudness: lm is NULL");
	return lm->timer.query (enable, ms, launches);
}

} /* extern "C" */
