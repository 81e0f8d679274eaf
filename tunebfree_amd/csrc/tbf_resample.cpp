/*
 * tbf_resample.cpp -- the host side of the output rate converter: tbf_resampler_set, the
 * tbf_render_resampled* / tbf_process_resampled* calls and the tbf_debug_resample* hooks.
 *
 * A post-stage on whatever L / R the chain delivers: the call's engine-rate pair is rendered
 * through the ordinary render path (plainRender, csrc/tbf_engine.cpp) and k_resample
 * (csrc/tbf_resample.hip) follows on the call's stream, where the pair is complete.  The stage is
 * this project's own (include/tbf.h): the reference renders at its host's
 * rate only.
 *
 * The host owns the position P of every instance (Instance::rsPos), so the counts of a call are
 * known before anything is launched and the call never waits for the device to learn them.
 * Scratch: with the caller's raw planes there is none.  Without them the pair goes to engine
 * scratch (tbf_engine.rotBuf), 8 B per instance and sample, and the call is cut into pieces of at
 * most TBF_STAGE_PIECE blocks, so the scratch never exceeds n x TBF_STAGE_PIECE x 128 x 8 B; the pieces
 * deliver what one call delivers, bit for bit, like any other cut.  -12 when the device cannot
 * hold it.
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <numeric>
#include <string>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_engine_impl.h"
#include "tbf_resample.h"

extern "C" int tbf_launch_resample (const tbf_rs_launch* P, hipStream_t stream);

using namespace tbf;

namespace {

/* I0 (x), the power series in double, to the last term that changes the sum */
double besselI0 (double x)
{
	const double q = x * x / 4.0;
	double       s = 1.0, term = 1.0;
	for (int k = 1; k < 500; k++) {
		term *= q / ((double)k * (double)k);
		s += term;
		if (term < s * 1e-20)
			break;
	}
	return s;
}

/* the prototype g[k], k = 0 .. L T - 1 (include/tbf.h), in double, rounded to float */
void buildPrototype (uint32_t L, uint32_t M, uint32_t T, std::vector<float>& g)
{
	const uint32_t N  = L * T;
	const double   s  = (double)std::max (L, M), fc = 0.45 / s, c = ((double)N - 1.0) / 2.0, beta = 10.0;
	const double   i0b = besselI0 (beta);
	g.resize (N);
	for (uint32_t k = 0; k < N; k++) {
		const double x = 2.0 * fc * ((double)k - c);
		const double sinc = x == 0.0 ? 1.0 : sin (M_PI * x) / (M_PI * x);
		const double u = N > 1 ? 2.0 * (double)k / ((double)N - 1.0) - 1.0 : 0.0;
		const double w = besselI0 (beta * sqrt (std::max (0.0, 1.0 - u * u))) / i0b;
		g[k]           = (float)((double)L * 2.0 * fc * sinc * w);
	}
}

uint64_t tableFingerprint (const std::vector<float>& g)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (float f : g) {
		uint32_t w;
		memcpy (&w, &f, 4);
		h = (h ^ w) * 0x100000001b3ull;
		h ^= h >> 29;
	}
	return h | 1u;
}

/* the phase-major table on the device, once */
int uploadTable (tbf_engine* e)
{
	tbf_engine::Resampler& r = e->rs;
	if (r.tabUp)
		return 0;
	if (r.tab.ensure (r.pm.size ()))
		return fail (-12, "out of device memory (resampler table)");
	HIPCHK (hipMemcpy (r.tab.p, r.pm.data (), r.pm.size () * sizeof (float), hipMemcpyHostToDevice));
	r.tabUp = true;
	return 0;
}

/* The checks of the resampled calls, all before anything renders or steps (in: the effects-only
 * calls' input rows); pointers are compared on the host only. */
int resampleArgs (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, bool fx, const float* in,
                  uint64_t inStride, const tbf_resampled_out* o)
{
	if (!e || !o || !o->L || !o->R || !o->counts || (fx && !in) || (nev && !ev))
		return fail (-22, "null argument");
	if (!o->rawL != !o->rawR)
		return fail (-22, "rawL and rawR: both or neither");
	const tbf_engine::Resampler& r = e->rs;
	if (!r.L)
		return fail (-22, "no resampler set (tbf_resampler_set)");
	if (fx != chainFx (e->cfg.chain_mode))
		return fail (-22, fx ? "tbf_process_resampled* needs an effects-only engine (TBF_CHAIN_FX*)"
		                     : "effects-only engine (TBF_CHAIN_FX*) has no tone generator to render: use tbf_process_resampled*");
	const uint64_t per    = (uint64_t)nblocks * TBF_BLK;
	const uint64_t frames = rs_count (per, r.L, r.M);
	if (per > UINT32_MAX || frames > UINT32_MAX)
		return fail (-22, "call too long: the counts are 32-bit");
	if (o->stride < frames)
		return fail (-22, "out->stride smaller than tbf_resampled_frames (nblocks)");
	if (o->rawL && o->raw_stride < per)
		return fail (-22, "out->raw_stride smaller than nblocks*128");
	if (fx && inStride < per)
		return fail (-22, "in_stride smaller than nblocks*128");
	const uint64_t n = e->inst.size ();
	{ /* every range against every other.  Without instances or blocks all are empty; with both,
	   * frames = ceil (per L / M) >= 1, so the resampled rows are never empty beside raw ones that are not */
		const Span g[5] = {rowsSpan (o->L, n, o->stride * 4, frames * 4), rowsSpan (o->R, n, o->stride * 4, frames * 4),
		                   rowsSpan (o->rawL, n, o->raw_stride * 4, per * 4), rowsSpan (o->rawR, n, o->raw_stride * 4, per * 4),
		                   rowsSpan (fx ? in : nullptr, n, inStride * 4, per * 4)};
		if (anyOverlap (g, 5))
			return fail (-22, "input, resampled and raw ranges overlap");
	}
	if (int rc = eventsInOrder (ev, nev))
		return rc;
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) cannot render");
	return 0;
}

/* One resampled call on device memory, after resampleArgs.  counts: host memory, always. */
int resampleDevice (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn, uint64_t inStride,
                    const tbf_resampled_out& o, hipStream_t s)
{
	tbf_engine::Resampler& r = e->rs;
	const uint32_t         n = (uint32_t)e->inst.size ();
	if (int rc = engineDevice (e)) /* the instances' history exists from here */
		return rc;
	if (int rc = uploadTable (e))
		return rc;
	if (n == 0 || nblocks == 0) { /* nothing renders and no event applies, as in every render call */
		std::fill_n (o.counts, n, 0u);
		return 0;
	}
	const bool     raw   = o.rawL != nullptr;
	const uint32_t piece = raw ? nblocks : std::min (nblocks, TBF_STAGE_PIECE);
	float *        pl = o.rawL, *pr = o.rawR;
	uint64_t       pstride = o.raw_stride;
	if (!raw) {
		const size_t plane = (size_t)n * piece * TBF_BLK;
		if (e->rotBuf.ensure (2 * plane)) {
			(void)hipGetLastError ();
			return fail (-12, "out of device memory (resampler scratch: 8 B per instance and sample of a piece)");
		}
		pl      = e->rotBuf.p;
		pr      = e->rotBuf.p + plane;
		pstride = (uint64_t)piece * TBF_BLK;
	}
	/* P at the call's start; equal positions (the common case) travel as kernel arguments */
	std::vector<uint64_t> pos0 (n), tab;
	bool                  uni = true;
	for (uint32_t i = 0; i < n; i++) {
		pos0[i] = e->inst[i].rsPos;
		uni     = uni && pos0[i] == pos0[0];
	}
	if (!uni && r.pos.ensure (2 * (size_t)n)) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (resampler positions)");
	}
	/* every allocation of the call has succeeded: only now the caller's counts are written */
	for (uint32_t i = 0; i < n; i++)
		o.counts[i] = (uint32_t)(rs_count (pos0[i] + (uint64_t)nblocks * TBF_BLK, r.L, r.M) - rs_count (pos0[i], r.L, r.M));
	for (Pieces pc (ev, nev, nblocks, piece); pc.next ();) {
		const uint32_t p0 = pc.p0, len = pc.len;
		tbf_rs_launch P;
		memset (&P, 0, sizeof (P));
		if (!uni) {
			/* per instance: read from a host vector of this call, so the stream is waited for before
			 * it changes: instances at different positions cost the call its overlap */
			tab.resize (2 * (size_t)n);
			for (uint32_t i = 0; i < n; i++) {
				tab[2 * (size_t)i]     = e->inst[i].rsPos;
				tab[2 * (size_t)i + 1] = pos0[i];
			}
			HIPCHK (hipMemcpyAsync (r.pos.p, tab.data (), tab.size () * sizeof (uint64_t), hipMemcpyHostToDevice, s));
			HIPCHK (hipStreamSynchronize (s));
			P.pos = r.pos.p;
		}
		const size_t off = raw ? (size_t)p0 * TBF_BLK : 0;
		if (int rc = plainRender (e, len, pc.npe ? pc.pe : nullptr, pc.npe, dIn ? dIn + (size_t)p0 * TBF_BLK : nullptr, inStride,
		                          pl + off, pr + off, pstride, s))
			return rc;
		P.in[0]      = pl + off;
		P.in[1]      = pr + off;
		P.inStride   = pstride;
		P.out[0]     = o.L;
		P.out[1]     = o.R;
		P.outStride  = o.stride;
		P.hist       = r.st.p;
		P.tab        = r.tab.p;
		P.posU       = e->inst[0].rsPos;
		P.pos0U      = pos0[0];
		P.n          = n;
		P.nIn        = len * TBF_BLK;
		P.L          = r.L;
		P.M          = r.M;
		P.T          = r.T;
		P.histFloats = r.histFloats ();
		P.TO         = r.TO;
		P.TS         = r.TS;
		P.winFloats  = r.winFloats;
		P.ldsRow     = r.ldsRow;
		StageTimer::Guard tg (r.timer, s, "resampler"); /* tbf_debug_resample_time: k_resample between two events on its stream */
		if (int rc = tg.begin ())
			return rc;
		if (tbf_launch_resample (&P, s))
			return fail (-5, std::string ("k_resample launch failed: ") + hipGetErrorString (hipGetLastError ()));
		if (int rc = tg.end ())
			return rc;
		r.launches++;
		for (uint32_t i = 0; i < n; i++)
			e->inst[i].rsPos += (uint64_t)len * TBF_BLK;
	}
	return 0;
}

/* the host-buffer calls: stage the input and the planes on the device, run, copy back */
int resampleHost (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t inStride, const tbf_resampled_out* o)
{
	HIPCHK (hipSetDevice (e->cfg.device));
	tbf_engine::Resampler& r   = e->rs;
	const uint32_t         n   = (uint32_t)e->inst.size ();
	const size_t           per = (size_t)nblocks * TBF_BLK, frames = (size_t)rs_count (per, r.L, r.M);
	if (n == 0 || per == 0) {
		std::fill_n (o->counts, n, 0u);
		return 0;
	}
	const size_t plane = (size_t)n * per, oplane = (size_t)n * frames;
	if (r.hostOut.ensure (2 * oplane) || (o->rawL && (e->outL.ensure (plane) || e->outR.ensure (plane))) ||
	    (in && e->extBuf.ensure (plane))) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (resampled outputs)");
	}
	if (in)
		if (int rc = stageHostInput (e->extBuf.p, in, inStride, per, n, e->stream))
			return rc;
	tbf_resampled_out d = {r.hostOut.p, r.hostOut.p + oplane, nullptr, nullptr, frames, per, o->counts};
	if (o->rawL) {
		d.rawL = e->outL.p;
		d.rawR = e->outR.p;
	}
	if (int rc = resampleDevice (e, nblocks, nullptr, 0, in ? e->extBuf.p : nullptr, per, d, e->stream))
		return rc;
	/* instance i's [0, counts[i]) alone: nothing else of the caller's rows is written */
	for (uint32_t i = 0; i < n; i++) {
		const size_t c = o->counts[i];
		if (!c)
			continue;
		HIPCHK (hipMemcpyAsync (o->L + i * o->stride, d.L + i * frames, c * 4, hipMemcpyDeviceToHost, e->stream));
		HIPCHK (hipMemcpyAsync (o->R + i * o->stride, d.R + i * frames, c * 4, hipMemcpyDeviceToHost, e->stream));
	}
	if (o->rawL) {
		HIPCHK (hipMemcpy2DAsync (o->rawL, o->raw_stride * 4, d.rawL, per * 4, per * 4, n, hipMemcpyDeviceToHost, e->stream));
		HIPCHK (hipMemcpy2DAsync (o->rawR, o->raw_stride * 4, d.rawR, per * 4, per * 4, n, hipMemcpyDeviceToHost, e->stream));
	}
	HIPCHK (hipStreamSynchronize (e->stream));
	return 0;
}

} // namespace

int tbf::resampleGrow (tbf_engine* e, uint32_t old, uint32_t n)
{
	tbf_engine::Resampler& r = e->rs;
	if (!r.L)
		return 0;
	const size_t  per = r.instFloats ();
	DevBuf<float> ns;
	if (ns.ensure ((size_t)n * per))
		return fail (-12, "out of device memory (resampler history)");
	if (old)
		HIPCHK (hipMemcpy (ns.p, r.st.p, (size_t)old * per * sizeof (float), hipMemcpyDeviceToDevice));
	HIPCHK (hipMemset (ns.p + (size_t)old * per, 0, (size_t)(n - old) * per * sizeof (float)));
	r.st = std::move (ns);
	return 0;
}

extern "C" {

int tbf_resampler_set (tbf_engine* e, uint32_t out_rate_hz)
{
	if (!e)
		return fail (-22, "null argument");
	if (e->everAdded || !e->inst.empty ())
		return fail (-16, "the resampler shapes the instances' state: set it before tbf_instances_add");
	tbf_engine::Resampler& r = e->rs;
	if (out_rate_hz == 0) {
		r = tbf_engine::Resampler ();
		return 0;
	}
	const double sr = e->cfg.sample_rate;
	if (!(sr >= 1.0) || sr > 4294967295.0 || sr != floor (sr))
		return fail (-22, "resampler: the engine's sample rate is not an integer number of Hz");
	const uint32_t Fi = (uint32_t)sr;
	if (out_rate_hz == Fi)
		return fail (-22, "resampler: the output rate equals the engine's rate");
	const uint32_t g = std::gcd (Fi, out_rate_hz);
	const uint64_t L = out_rate_hz / g, M = Fi / g, s = std::max (L, M);
	uint64_t       T = (2ull * TBF_RS_ZC * s + L - 1) / L;
	T += T & 1u;
	if (L > TBF_RS_MAX_L || L * T > TBF_RS_MAX_TABLE)
		return fail (-22, "resampler: ratio " + std::to_string (L) + " / " + std::to_string (M) +
		                      " beyond the cap (L <= 1024, L * T <= 2^18)");
	tbf_engine::Resampler nr;
	nr.Fo = out_rate_hz;
	nr.L  = (uint32_t)L;
	nr.M  = (uint32_t)M;
	nr.T  = (uint32_t)T;
	buildPrototype (nr.L, nr.M, nr.T, nr.g);
	nr.fp = tableFingerprint (nr.g);
	const uint32_t row = TBF_RS_ROW (nr.T);
	nr.pm.assign ((size_t)nr.L * row, 0.0f);
	for (uint32_t p = 0; p < nr.L; p++)
		for (uint32_t t = 0; t < nr.T; t++)
			nr.pm[(size_t)p * row + t] = nr.g[p + (size_t)t * nr.L];
	/* the tile: as many outputs as the lanes carry while their newest inputs leave the window room
	 * for taps (at least half of it), then as many taps a segment as fit (csrc/tbf_resample.hip);
	 * the table goes to LDS when its rows fit there at an odd stride */
	uint32_t TO = TBF_RS_LANES * TBF_RS_PER_LANE;
	auto     span = [&] (uint32_t to) { return (uint32_t)(((L - 1) + (uint64_t)(to - 1) * M) / L + 1); };
	while (TO > 1 && span (TO) > TBF_RS_WINDOW / 2)
		TO /= 2;
	nr.TO        = TO;
	nr.TS        = std::min<uint32_t> (nr.T, TBF_RS_WINDOW - span (TO) + 1);
	nr.winFloats = span (TO) + nr.TS - 1;
	nr.ldsRow    = (L > 1 && L * (nr.T | 1u) <= TBF_RS_TAB_LDS) ? (nr.T | 1u) : 0;
	r     = std::move (nr);
	return 0;
}

int tbf_resampled_frames (const tbf_engine* e, uint32_t nblocks, uint64_t* max_frames)
{
	if (!e || !max_frames)
		return fail (-22, "null argument");
	if (!e->rs.L)
		return fail (-22, "no resampler set (tbf_resampler_set)");
	*max_frames = rs_count ((uint64_t)nblocks * TBF_BLK, e->rs.L, e->rs.M);
	return 0;
}

int tbf_render_resampled (tbf_engine* e, uint32_t nblocks, const tbf_resampled_out* out)
{
	if (int rc = resampleArgs (e, nblocks, nullptr, 0, false, nullptr, 0, out))
		return rc;
	return resampleHost (e, nblocks, nullptr, 0, out);
}

int tbf_render_resampled_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev,
                                 const tbf_resampled_out* out, void* stream)
{
	if (int rc = resampleArgs (e, nblocks, ev, nev, false, nullptr, 0, out))
		return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	return resampleDevice (e, nblocks, ev, nev, nullptr, 0, *out, streamOr (stream, e->stream));
}

int tbf_process_resampled (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t inStride, const tbf_resampled_out* out)
{
	if (int rc = resampleArgs (e, nblocks, nullptr, 0, true, in, inStride, out))
		return rc;
	return resampleHost (e, nblocks, in, inStride, out);
}

int tbf_process_resampled_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn,
                                  uint64_t inStride, const tbf_resampled_out* out, void* stream)
{
	if (int rc = resampleArgs (e, nblocks, ev, nev, true, dIn, inStride, out))
		return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	return resampleDevice (e, nblocks, ev, nev, dIn, inStride, *out, streamOr (stream, e->stream));
}

int tbf_debug_resampler (const tbf_engine* e, uint32_t* L, uint32_t* M, uint32_t* T, float* table, uint64_t cap,
                         double* latency)
{
	if (!e)
		return fail (-22, "null argument");
	const tbf_engine::Resampler& r = e->rs;
	if (L)
		*L = r.L;
	if (M)
		*M = r.M;
	if (T)
		*T = r.T;
	if (latency)
		*latency = r.L ? ((double)r.g.size () - 1.0) / (2.0 * r.L) : 0.0;
	if (table) {
		if (cap < r.g.size ())
			return fail (-22, "resampler table: " + std::to_string (r.g.size ()) + " floats, capacity " + std::to_string (cap));
		std::copy (r.g.begin (), r.g.end (), table);
	}
	return 0;
}

int tbf_debug_resample_ref (const tbf_engine* e, const float* x, uint64_t n_in, const float* hist, uint64_t pos0, float* y,
                            uint64_t cap, uint64_t* n_out)
{
	if (!e || (n_in && !x))
		return fail (-22, "null argument");
	const tbf_engine::Resampler& r = e->rs;
	if (!r.L)
		return fail (-22, "no resampler set (tbf_resampler_set)");
	const uint64_t n0 = rs_count (pos0, r.L, r.M), n1 = rs_count (pos0 + n_in, r.L, r.M);
	if (n_out)
		*n_out = n1 - n0;
	if (n1 == n0)
		return 0;
	if (!y || cap < n1 - n0)
		return fail (-22, "resample_ref: " + std::to_string (n1 - n0) + " outputs, capacity " + std::to_string (cap));
	const uint32_t     H = r.T - 1, row = TBF_RS_ROW (r.T);
	std::vector<float> buf (H + n_in, 0.0f); /* the history, then samples pos0 .. */
	if (hist)
		std::copy (hist, hist + H, buf.begin ());
	std::copy (x, x + n_in, buf.begin () + H);
	for (uint64_t n = n0; n < n1; n++) {
		const uint64_t p = n * r.M, i = p / r.L;
		const uint32_t phi = (uint32_t)(p - i * r.L);
		y[n - n0]          = rs_taps (0.0f, r.pm.data () + (size_t)phi * row, buf.data () + H + (i - pos0), r.T);
	}
	return 0;
}

int tbf_debug_resampler_pos (tbf_engine* e, uint32_t inst, uint64_t pos)
{
	if (!e)
		return fail (-22, "null argument");
	if (inst >= e->inst.size ())
		return fail (-22, "instance " + std::to_string (inst) + " does not exist");
	e->inst[inst].rsPos = pos;
	return 0;
}

int tbf_debug_resample_time (tbf_engine* e, int32_t enable, double* ms, uint64_t* launches)
{
	if (!e)
		return fail (-22, "null argument");
	return e->rs.timer.query (enable, ms, launches);
}

} /* extern "C" */
