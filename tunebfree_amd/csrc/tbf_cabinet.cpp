/*
 * tbf_cabinet.cpp -- the host side of the cabinet convolver: tbf_cabinet_set, the
 * tbf_render_cabinet* / tbf_process_cabinet* calls and tbf_debug_cabinet.
 *
 * The reference's JACK host in its convolver build runs whirlProc2, sends the horn pair
 * through an impulse response and mixes the drum pair in afterwards (src/main.cpp:265-281).
 * Here that is one call: the rotor planes of the call are rendered through the rotor path
 * (rotorRender, csrc/tbf_engine.cpp) and k_cabinet (csrc/tbf_cabinet.hip) follows on the
 * call's stream, where the planes are complete.  The convolver's arithmetic and the mix law are
 * this project's own: the reference tree has no convolver source.
 *
 * Scratch: with the caller's rotor planes (rotors != NULL) there is none.  Without them the
 * four planes go to engine scratch (tbf_engine.rotBuf), 16 B per instance and sample, and the
 * call is cut into pieces of at most TBF_STAGE_PIECE blocks, so the scratch never exceeds
 * n x TBF_STAGE_PIECE x 128 x 16 B (2.1 GB at 4096 instances); the pieces render what one call
 * renders, bit for bit, like any other cut.  -12 when the device cannot hold it.
 * The mix (convolution.mix) is a host control: k_cabinet reads it per instance (wet0, uploaded
 * when it changed) or, in a call in which a mix event lands, per instance and block (wetBlk).
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_cabinet.h"
#include "tbf_engine_impl.h"

extern "C" int tbf_launch_cabinet (const tbf_cab_launch* P, hipStream_t stream);
extern "C" int tbf_chain_stages (uint32_t chain);

using namespace tbf;

namespace {

bool chainWhirl (uint32_t chain) { return tbf_chain_stages (chain) == TBF_NSTAGES; }

/* H_k = FFT-256 of taps [128 k, 128 k + 128) zero-padded, in double, rounded to float, packed
 * (csrc/tbf_cabinet.h); tw: cos and -sin of 2 pi j / 256 */
void buildTables (const std::vector<float>& ir, uint32_t K, std::vector<float>& H)
{
	double c[TBF_CAB_FFT], s[TBF_CAB_FFT];
	for (int j = 0; j < TBF_CAB_FFT; j++) {
		c[j] = cos (2.0 * M_PI * j / TBF_CAB_FFT);
		s[j] = sin (2.0 * M_PI * j / TBF_CAB_FFT);
	}
	H.assign ((size_t)K * 256, 0.0f);
	for (uint32_t k = 0; k < K; k++) {
		const size_t   t0 = (size_t)k * TBF_CAB_PART;
		const uint32_t nt = (uint32_t)std::min<size_t> (TBF_CAB_PART, ir.size () - t0);
		for (uint32_t j = 0; j <= 128; j++) {
			double re = 0.0, im = 0.0;
			for (uint32_t t = 0; t < nt; t++) {
				const uint32_t a = (j * t) & (TBF_CAB_FFT - 1);
				re += (double)ir[t0 + t] * c[a];
				im -= (double)ir[t0 + t] * s[a];
			}
			float* h = H.data () + (size_t)k * 256;
			if (j == 0)
				h[0] = (float)re;
			else if (j == 128)
				h[1] = (float)re;
			else {
				h[2 * j]     = (float)re;
				h[2 * j + 1] = (float)im;
			}
		}
	}
}

uint64_t tapsFingerprint (const std::vector<float>& l, const std::vector<float>& r)
{
	uint64_t h = 0xcbf29ce484222325ull;
	for (const std::vector<float>* v : {&l, &r})
		for (float f : *v) {
			uint32_t w;
			memcpy (&w, &f, 4);
			h = (h ^ w) * 0x100000001b3ull;
			h ^= h >> 29;
		}
	return h | 1u;
}

/* the response's tables on the device, once */
int uploadTables (tbf_engine* e)
{
	tbf_engine::Cabinet& c = e->cab;
	if (c.tablesUp)
		return 0;
	std::vector<float> tw (256);
	for (int j = 0; j < 128; j++) {
		tw[j]       = (float)cos (2.0 * M_PI * j / TBF_CAB_FFT);
		tw[128 + j] = (float)-sin (2.0 * M_PI * j / TBF_CAB_FFT);
	}
	if (c.tw.ensure (256) || c.H[0].ensure ((size_t)c.K * 256) || c.H[1].ensure ((size_t)c.K * 256))
		return fail (-12, "out of device memory (cabinet tables)");
	HIPCHK (hipMemcpy (c.tw.p, tw.data (), 256 * sizeof (float), hipMemcpyHostToDevice));
	std::vector<float> H;
	for (int ch = 0; ch < 2; ch++) {
		buildTables (c.ir[ch], c.K, H);
		HIPCHK (hipMemcpy (c.H[ch].p, H.data (), H.size () * sizeof (float), hipMemcpyHostToDevice));
	}
	c.tablesUp = true;
	return 0;
}

/* The checks of the cabinet calls, all before anything renders or steps (in: the effects-only
 * calls' input rows); pointers are compared on the host only. */
int cabinetArgs (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, bool fx, const float* in,
                 uint64_t inStride, const tbf_cabinet_out* cab, const tbf_rotor_out* rot)
{
	if (!e || !cab || !cab->L || !cab->R || (fx && !in) || (nev && !ev))
		return fail (-22, "null argument");
	if (!cab->wetL != !cab->wetR)
		return fail (-22, "wetL and wetR: both or neither");
	if (rot && (!rot->hornL || !rot->hornR || !rot->drumL || !rot->drumR))
		return fail (-22, "rotors: all four planes or a NULL rotors");
	if (!e->cab.K)
		return fail (-22, "no cabinet set (tbf_cabinet_set)");
	if (fx != chainFx (e->cfg.chain_mode))
		return fail (-22, fx ? "tbf_process_cabinet* needs an effects-only engine (TBF_CHAIN_FX)"
		                     : "effects-only engine (TBF_CHAIN_FX) has no tone generator to render: use tbf_process_cabinet*");
	const uint64_t per = (uint64_t)nblocks * TBF_BLK;
	if (cab->stride < per)
		return fail (-22, "cab->stride smaller than nblocks*128");
	if (rot && rot->stride < per)
		return fail (-22, "rotors->stride smaller than nblocks*128");
	if (fx && inStride < per)
		return fail (-22, "in_stride smaller than nblocks*128");
	const uint64_t n = e->inst.size ();
	{ /* every range against every other; an absent wet pair is empty, and without instances or blocks all are */
		Span r[9];
		int  nr = 0;
		for (const float* p : {cab->L, cab->R, cab->wetL, cab->wetR})
			r[nr++] = rowsSpan (p, n, cab->stride * 4, per * 4);
		if (rot)
			for (const float* p : {rot->hornL, rot->hornR, rot->drumL, rot->drumR})
				r[nr++] = rowsSpan (p, n, rot->stride * 4, per * 4);
		if (fx)
			r[nr++] = rowsSpan (in, n, inStride * 4, per * 4);
		if (anyOverlap (r, nr))
			return fail (-22, "input, cabinet and rotor ranges overlap");
	}
	if (int rc = eventsInOrder (ev, nev))
		return rc;
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) cannot render");
	return 0;
}

/* the mix the piece's k_cabinet reads: per instance as the instances hold it now (uploaded when
 * it differs from what the device has), and per (instance, block) when one of the piece's
 * events [ev, ev + nev) sets convolution.mix before block len.  The uploads read host vectors
 * of this call, so the stream is waited for before they go out of scope: a mix change costs
 * the call its overlap with the work before it, a steady mix costs nothing. */
int stageMix (tbf_engine* e, const tbf_event* ev, uint32_t nev, uint32_t len, hipStream_t s, tbf_cab_launch& P)
{
	tbf_engine::Cabinet& c = e->cab;
	const uint32_t       n = (uint32_t)e->inst.size ();
	std::vector<float>   w (n);
	for (uint32_t i = 0; i < n; i++)
		w[i] = e->inst[i].cabWet;
	bool sync = false;
	if (w != c.wetDev || c.wet0.cap < n) {
		if (c.wet0.ensure (n))
			return fail (-12, "out of device memory (cabinet mix)");
		HIPCHK (hipMemcpyAsync (c.wet0.p, w.data (), n * sizeof (float), hipMemcpyHostToDevice, s));
		c.wetDev = w;
		sync     = true;
	}
	P.wet0   = c.wet0.p;
	P.wetBlk = nullptr;
	const int          mixId = tbf_midi_control_id ("convolution.mix");
	std::vector<float> tab;
	for (uint32_t k = 0; k < nev && ev[k].block < len; k++) {
		const tbf_event& v = ev[k];
		if (v.kind != TBF_EV_CONTROL || v.id != mixId || v.inst >= n || (int)v.value < 0)
			continue;
		if (tab.empty ()) {
			tab.resize ((size_t)n * len);
			for (uint32_t i = 0; i < n; i++)
				std::fill_n (tab.begin () + (size_t)i * len, len, w[i]);
		}
		std::fill (tab.begin () + (size_t)v.inst * len + v.block, tab.begin () + (size_t)(v.inst + 1) * len,
		           cabinetWet ((int)v.value));
	}
	if (!tab.empty ()) {
		if (c.wetBlk.ensure (tab.size ()))
			return fail (-12, "out of device memory (cabinet mix)");
		HIPCHK (hipMemcpyAsync (c.wetBlk.p, tab.data (), tab.size () * sizeof (float), hipMemcpyHostToDevice, s));
		P.wetBlk = c.wetBlk.p;
		sync     = true;
	}
	if (sync)
		HIPCHK (hipStreamSynchronize (s));
	return 0;
}

/* One cabinet call on device memory, after cabinetArgs. */
int cabinetDevice (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn, uint64_t inStride,
                   const tbf_cabinet_out& cab, const tbf_rotor_out* rot, hipStream_t s)
{
	if (int rc = engineDevice (e)) /* the instances' history exists from here */
		return rc;
	if (int rc = uploadTables (e))
		return rc;
	tbf_engine::Cabinet& c = e->cab;
	const uint32_t       n = (uint32_t)e->inst.size ();
	if (n == 0 || nblocks == 0) /* nothing renders and no event applies, as in every render call */
		return 0;
	const uint32_t piece = rot ? nblocks : std::min (nblocks, TBF_STAGE_PIECE);
	tbf_rotor_out  planes;
	if (rot)
		planes = *rot;
	else {
		const size_t plane = (size_t)n * piece * TBF_BLK;
		if (e->rotBuf.ensure (4 * plane)) {
			(void)hipGetLastError ();
			return fail (-12, "out of device memory (cabinet scratch: 16 B per instance and sample of a piece)");
		}
		planes = {e->rotBuf.p, e->rotBuf.p + plane, e->rotBuf.p + 2 * plane, e->rotBuf.p + 3 * plane, (uint64_t)piece * TBF_BLK};
	}
	for (Pieces pc (ev, nev, nblocks, piece); pc.next ();) {
		const uint32_t p0 = pc.p0, len = pc.len;
		tbf_cab_launch P;
		memset (&P, 0, sizeof (P));
		if (int rc = stageMix (e, pc.pe, pc.npe, len, s, P))
			return rc;
		if (int rc = rotorRender (e, len, pc.npe ? pc.pe : nullptr, pc.npe, dIn ? dIn + (size_t)p0 * TBF_BLK : nullptr, inStride,
		                          planes, s))
			return rc;
		const size_t off = (size_t)p0 * TBF_BLK;
		P.horn[0]   = planes.hornL;
		P.horn[1]   = planes.hornR;
		P.drum[0]   = planes.drumL;
		P.drum[1]   = planes.drumR;
		P.rotStride = planes.stride;
		P.out[0]    = cab.L + off;
		P.out[1]    = cab.R + off;
		P.wet[0]    = cab.wetL ? cab.wetL + off : nullptr;
		P.wet[1]    = cab.wetR ? cab.wetR + off : nullptr;
		P.outStride = cab.stride;
		P.state     = c.st.p;
		P.chFloats  = TBF_CAB_CH_FLOATS (c.K);
		P.H[0]      = c.H[0].p;
		P.H[1]      = c.H[1].p;
		P.tw        = c.tw.p;
		P.n         = n;
		P.nb        = len;
		P.K         = c.K;
		P.R         = TBF_CAB_RING (c.K);
		StageTimer::Guard tg (c.timer, s, "cabinet"); /* tbf_debug_cabinet_time: k_cabinet between two events on its stream */
		if (int rc = tg.begin ())
			return rc;
		if (tbf_launch_cabinet (&P, s))
			return fail (-5, std::string ("k_cabinet launch failed: ") + hipGetErrorString (hipGetLastError ()));
		if (int rc = tg.end ())
			return rc;
		c.launches++;
	}
	return 0;
}

/* the host-buffer calls: stage the input and the planes on the device, run, copy back */
int cabinetHost (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t inStride, const tbf_cabinet_out* cab,
                 const tbf_rotor_out* rot)
{
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t n   = (uint32_t)e->inst.size ();
	const size_t   per = (size_t)nblocks * TBF_BLK;
	if (n == 0 || per == 0)
		return 0;
	const size_t plane = (size_t)n * per;
	const int    extra = (cab->wetL ? 2 : 0) + (rot ? 4 : 0);
	if (e->outL.ensure (plane) || e->outR.ensure (plane) || (extra && e->cab.hostOut.ensure (extra * plane)) ||
	    (in && e->extBuf.ensure (plane))) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (cabinet outputs)");
	}
	if (in)
		if (int rc = stageHostInput (e->extBuf.p, in, inStride, per, n, e->stream))
			return rc;
	float*          x = e->cab.hostOut.p;
	tbf_cabinet_out dc = {e->outL.p, e->outR.p, nullptr, nullptr, per};
	if (cab->wetL) {
		dc.wetL = x;
		dc.wetR = x + plane;
		x += 2 * plane;
	}
	const tbf_rotor_out dr = {x, x + plane, x + 2 * plane, x + 3 * plane, per};
	if (int rc = cabinetDevice (e, nblocks, nullptr, 0, in ? e->extBuf.p : nullptr, per, dc, rot ? &dr : nullptr, e->stream))
		return rc;
	auto back = [&] (float* host, uint64_t stride, const float* dev) {
		return hipMemcpy2DAsync (host, stride * 4, dev, per * 4, per * 4, n, hipMemcpyDeviceToHost, e->stream);
	};
	HIPCHK (back (cab->L, cab->stride, dc.L));
	HIPCHK (back (cab->R, cab->stride, dc.R));
	if (cab->wetL) {
		HIPCHK (back (cab->wetL, cab->stride, dc.wetL));
		HIPCHK (back (cab->wetR, cab->stride, dc.wetR));
	}
	if (rot) {
		HIPCHK (back (rot->hornL, rot->stride, dr.hornL));
		HIPCHK (back (rot->hornR, rot->stride, dr.hornR));
		HIPCHK (back (rot->drumL, rot->stride, dr.drumL));
		HIPCHK (back (rot->drumR, rot->stride, dr.drumR));
	}
	HIPCHK (hipStreamSynchronize (e->stream));
	return 0;
}

} // namespace

int tbf::cabinetGrow (tbf_engine* e, uint32_t old, uint32_t n)
{
	tbf_engine::Cabinet& c = e->cab;
	if (!c.K)
		return 0;
	const size_t  per = c.instFloats ();
	DevBuf<float> ns;
	if (ns.ensure ((size_t)n * per))
		return fail (-12, "out of device memory (cabinet history)");
	if (old)
		HIPCHK (hipMemcpy (ns.p, c.st.p, (size_t)old * per * sizeof (float), hipMemcpyDeviceToDevice));
	HIPCHK (hipMemset (ns.p + (size_t)old * per, 0, (size_t)(n - old) * per * sizeof (float)));
	c.st = std::move (ns);
	return 0;
}

extern "C" {

int tbf_cabinet_set (tbf_engine* e, const float* irL, const float* irR, uint32_t taps)
{
	if (!e)
		return fail (-22, "null argument");
	if (taps > TBF_CAB_MAX_TAPS)
		return fail (-22, "cabinet response longer than TBF_CAB_MAX_TAPS");
	if (taps && (!irL || !irR))
		return fail (-22, "null impulse response");
	for (uint32_t t = 0; t < taps; t++)
		if (!std::isfinite (irL[t]) || !std::isfinite (irR[t]))
			return fail (-22, "cabinet response: tap " + std::to_string (t) + " is not finite");
	if (taps && !chainWhirl (e->cfg.chain_mode))
		return fail (-22, "a cabinet needs a chain that runs the whirl (TBF_CHAIN_FULL, TBF_CHAIN_FX)");
	if (e->everAdded || !e->inst.empty ())
		return fail (-16, "the cabinet shapes the instances' state: set it before tbf_instances_add");
	tbf_engine::Cabinet& c = e->cab;
	c.taps     = taps;
	c.K        = (taps + TBF_CAB_PART - 1) / TBF_CAB_PART;
	c.ir[0].assign (irL, irL + taps);
	c.ir[1].assign (irR, irR + taps);
	c.fp       = taps ? tapsFingerprint (c.ir[0], c.ir[1]) : 0;
	c.tablesUp = false;
	return 0;
}

int tbf_render_cabinet (tbf_engine* e, uint32_t nblocks, const tbf_cabinet_out* cab, const tbf_rotor_out* rotors)
{
	if (int rc = cabinetArgs (e, nblocks, nullptr, 0, false, nullptr, 0, cab, rotors))
		return rc;
	return cabinetHost (e, nblocks, nullptr, 0, cab, rotors);
}

int tbf_render_cabinet_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const tbf_cabinet_out* cab,
                               const tbf_rotor_out* rotors, void* stream)
{
	if (int rc = cabinetArgs (e, nblocks, ev, nev, false, nullptr, 0, cab, rotors))
		return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	return cabinetDevice (e, nblocks, ev, nev, nullptr, 0, *cab, rotors, streamOr (stream, e->stream));
}

int tbf_process_cabinet (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t inStride, const tbf_cabinet_out* cab,
                         const tbf_rotor_out* rotors)
{
	if (int rc = cabinetArgs (e, nblocks, nullptr, 0, true, in, inStride, cab, rotors))
		return rc;
	return cabinetHost (e, nblocks, in, inStride, cab, rotors);
}

int tbf_process_cabinet_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn,
                                uint64_t inStride, const tbf_cabinet_out* cab, const tbf_rotor_out* rotors, void* stream)
{
	if (int rc = cabinetArgs (e, nblocks, ev, nev, true, dIn, inStride, cab, rotors))
		return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	return cabinetDevice (e, nblocks, ev, nev, dIn, inStride, *cab, rotors, streamOr (stream, e->stream));
}

int tbf_debug_cabinet_time (tbf_engine* e, int32_t enable, double* ms, uint64_t* launches)
{
	if (!e)
		return fail (-22, "null argument");
	return e->cab.timer.query (enable, ms, launches);
}

int tbf_debug_cabinet (const tbf_engine* e, uint32_t inst, uint32_t* taps, uint32_t* parts, uint64_t* inst_bytes,
                       uint64_t* launches, float* wet)
{
	if (!e)
		return fail (-22, "null argument");
	if (wet) {
		if (inst >= e->inst.size ())
			return fail (-22, "instance " + std::to_string (inst) + " does not exist");
		*wet = e->inst[inst].cabWet;
	}
	if (taps)
		*taps = e->cab.taps;
	if (parts)
		*parts = e->cab.K;
	if (inst_bytes)
		*inst_bytes = e->cab.instFloats () * sizeof (float);
	if (launches)
		*launches = e->cab.launches;
	return 0;
}

} /* extern "C" */
