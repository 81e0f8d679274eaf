/*
 * tbf_hostctl.cpp -- a render chunk's host control: hostControl
 * finds and scans the chunk's events, then stepChunkFront, stepChunkParallel or stepChunkSerial
 * applies them and steps the instances' control into the chunk's staging set.  Host logic
 * only, no HIP call.  Stated once here: what a parameter does (paramTab), the effect fields
 * of a control entry (effectFields), a device-control delta (emitDelta).
 */
#include <assert.h>
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <chrono>

#include "tbf_engine_impl.h"

typedef tbf_engine::ParStep ParStep;

/* What each TBF_P_* index does, one row each: the setter (src/clap.cpp:108-121
 * setToneGenParam + 162-207 setParam; k = index - first, a drawbar's bus; params[] holds the
 * value already) and what the device front end (k_front) gets for it: the event word's op
 * and, for an effect setter (TBF_FEV_EFFECT), TBF_FX_*, the values [lo, hi] the front end
 * takes -- outside the setter's sane range, or NaN, the chunk is the host front end's -- and
 * the value k_front receives in fevVal, read back from the instance after the setter (sent).
 * setParam, frontParam and the front-end mirror read nothing else: a change is one row. */
struct ParamRow {
	int32_t first, last;
	uint8_t op, fx;
	float   lo, hi;
	void (*set) (Instance& in, int32_t k, float v);
	float (*sent) (const Instance& in, float v);
};
#define SET(body) [] (Instance& in, int32_t k, float v) { body; }
#define SENT(expr) [] (const Instance& in, float v) -> float { return expr; }
#define R_SMALL -999999.9375f, 999999.9375f /* |v| < 1e6: the integer the setter derives is exact */
#define FX(x) TBF_FEV_EFFECT, TBF_FX_##x
static constexpr ParamRow paramTab[] = {
    {TBF_P_DRAWBAR_MIN, TBF_P_DRAWBAR_MAX, TBF_FEV_DRAWBAR, 0, 0, 0, SET (in.tg.setDrawBar (k, (unsigned)rint (v))), nullptr},
    {TBF_P_VIBRATO, TBF_P_VIBRATO, TBF_FEV_VIB_UPPER, 0, 0, 0, SET (in.tg.setVibratoUpper ((int)rint (v))), nullptr},
    {TBF_P_VIBRATO_TYPE, TBF_P_VIBRATO_TYPE, FX (VIBTYPE), R_SMALL, SET (in.tg.setVibratoFromInt ((int)floor (v))),
     SENT ((float)(int)floor (v))},
    /* the rotary option, a one-shot, from both parameters */
    {TBF_P_DRUM, TBF_P_HORN, FX (ROTOR), R_SMALL,
     SET (in.revOpt = (int)(floor (in.params[TBF_P_DRUM]) + 3 * floor (in.params[TBF_P_HORN]))), SENT ((float)in.revOpt)},
    {TBF_P_OVERDRIVE, TBF_P_OVERDRIVE, FX (CLEAN), R_SMALL, SET (in.odClean = (int)rint (1.0f - v)), SENT ((float)in.odClean)},
    {TBF_P_CHARACTER, TBF_P_CHARACTER, FX (CHARACTER), 0.0f, 1.0f, SET (setCharacter (in, v)), SENT (in.odA)},
    {TBF_P_REVERB, TBF_P_REVERB, FX (REVERB), -FLT_MAX, FLT_MAX, SET (in.rvG = v), SENT (in.rvG)},
    {TBF_P_PERCUSSION, TBF_P_PERCUSSION, TBF_FEV_PERC, 0, 0, 0, SET (in.tg.setPercEnabled ((int)rint (v))), nullptr},
    {TBF_P_PERCUSSION_VOLUME, TBF_P_PERCUSSION_VOLUME, FX (PERC_SOFT), R_SMALL, SET (in.tg.setPercVolume ((int)(1 - rint (v)))),
     SENT (in.tg.percIsSoft != 0 ? 1.0f : 0.0f)},
    {TBF_P_PERCUSSION_DECAY, TBF_P_PERCUSSION_DECAY, FX (PERC_FAST), R_SMALL, SET (in.tg.setPercFast ((int)rint (v))),
     SENT (in.tg.percIsFast != 0 ? 1.0f : 0.0f)},
    {TBF_P_PERCUSSION_HARMONIC, TBF_P_PERCUSSION_HARMONIC, TBF_FEV_PERC_FIRST, 0, 0, 0, SET (in.tg.setPercFirst ((int)rint (v))),
     nullptr},
    {TBF_P_BUS_DRAWBAR_BASE, TBF_P_BUS_DRAWBAR_BASE + 26, TBF_FEV_DRAWBAR, 0, 0, 0,
     SET (in.tg.setDrawBar (k, (unsigned)rint (v))), nullptr},
    {TBF_P_VIBRATO_LOWER, TBF_P_VIBRATO_LOWER, TBF_FEV_VIB_LOWER, 0, 0, 0, SET (in.tg.setVibratoLower ((int)rint (v))), nullptr},
    {TBF_P_SWELL, TBF_P_SWELL, FX (SWELL), 0.0f, 2.0f,
     SET (in.tg.swellPedalGain = (float)((in.tg.outputLevelTrim * ((double)(unsigned char)rint (v * 127.0))) / 127.0)),
     SENT (in.tg.swellPedalGain)},
    {TBF_P_WHIRL_BYPASS, TBF_P_WHIRL_BYPASS, FX (BYPASS), R_SMALL, SET (in.whBypass = (int)rint (v)), SENT ((float)in.whBypass)},
};

#undef SET
#undef SENT
#undef R_SMALL
#undef FX
static_assert (TBF_P_HORN == TBF_P_DRUM + 1, "the rotor row spans both parameters");
static_assert (TBF_P_WHIRL_BYPASS == 132 && TBF_P_WHIRL_BYPASS > TBF_P_BUS_DRAWBAR_BASE + 26, "the largest index sizes ParamIndex");

/* the row of an index (-1: none), built at compile time */
static constexpr struct ParamIndex {
	int8_t of[TBF_P_WHIRL_BYPASS + 1] = {};
	constexpr ParamIndex ()
	{
		for (int8_t& r : of)
			r = -1;
		for (size_t r = 0; r < sizeof (paramTab) / sizeof (paramTab[0]); r++)
			for (int32_t i = paramTab[r].first; i <= paramTab[r].last; i++)
				of[i] = (int8_t)r;
	}
} paramIndex;

static inline const ParamRow* paramRow (int32_t index)
{
	return index >= 0 && index <= TBF_P_WHIRL_BYPASS && paramIndex.of[index] >= 0 ? &paramTab[paramIndex.of[index]] : nullptr;
}

/* tbf_set_param's effect on the instance and nothing else (no markActive, no ctlDirty);
 * false for an index that is no parameter */
bool tbf::setParam (Instance& in, int32_t index, float value)
{
	const bool stored = index >= 0 && index < 64;
	if (stored)
		in.params[index] = value;
	const ParamRow* r = paramRow (index);
	if (r)
		r->set (in, index - r->first, value);
	return r || stored;
}

/* a parameter event the device front end steps, as a TBF_FEV_* word without the block; 0
 * for any other.  Drawbars and the vibrato and percussion switches change what a control
 * record carries, the effect setters the entry's effect fields. */
static uint32_t frontParam (int32_t index, float v)
{
	const ParamRow* r = paramRow (index);
	if (!r)
		return 0;
	if (r->op == TBF_FEV_EFFECT)
		return v >= r->lo && v <= r->hi ? TBF_FEV_PARAM | (TBF_FEV_EFFECT << 12) | r->fx : 0;
	if (r->op == TBF_FEV_DRAWBAR) {
		const unsigned st = (unsigned)rint (v); /* as the setter hands it to setDrawBar */
		return TBF_FEV_PARAM | (TBF_FEV_DRAWBAR << 12) | ((st > 8 ? 15u : st) << 5) | (uint32_t)(index - r->first);
	}
	const uint32_t fl = (int)rint (v) != 0 ? 1u : 0u; /* the switches */
	return TBF_FEV_PARAM | ((uint32_t)r->op << 12) | (fl << 9);
}

/* a scheduled event (tbf_render_events) at its block boundary */
int tbf::applyEvent (tbf_engine* e, const tbf_event& ev)
{
	if (ev.inst >= e->inst.size ())
		return fail (-22, "event for a bad instance");
	switch (ev.kind) {
		case TBF_EV_NOTE: return tbf_note (e, ev.inst, ev.id, ev.value != 0.0);
		case TBF_EV_PARAM: return tbf_set_param (e, ev.inst, ev.id, ev.value);
		case TBF_EV_CONTROL:
			if (controlById (e->inst[ev.inst], ev.id, (int)ev.value) < 0)
				return fail (-22, "bad control function id");
			return 0;
		case TBF_EV_PROGRAM: return tbf_program_install (e, ev.inst, (uint32_t)ev.id);
		default: return fail (-22, "bad event kind");
	}
}

/* preamp per-block constants, src/overdrive.cpp:64-84 and the density/out loops */
static void odCtlCompute (const Instance& in, double sr, tbf_seg_ctl& c)
{
	double overallscale = 1.0;
	overallscale /= 44100.0;
	overallscale *= sr;
	double density = in.odA * 4.0;
	c.odIir        = pow (in.odB, 3) / overallscale;
	c.odOutput     = in.odC;
	c.odWet        = in.odD;
	c.odDry        = 1.0 - c.odWet;
	double out     = fabs (density);
	density        = density * fabs (density);
	double count   = density;
	int    iter    = 0;
	while (count > 1.0) {
		iter++;
		count = count - 1.0;
	}
	while (out > 1.0)
		out = out - 1.0;
	c.odIter       = iter;
	c.odOut        = out;
	c.odDensityPos = density > 0 ? 1u : 0u;
	c.odClean      = (uint32_t)in.odClean;
}

/* the preamp fields of a control entry, recomputed only when the preamp parameters changed
 * (the pow above costs more than the rest of a dense-event step per instance and block) */
static void odCtl (Instance& in, double sr, tbf_seg_ctl& c)
{
	Instance::OdCache& k = in.odc;
	if (!k.valid || k.A != in.odA || k.B != in.odB || k.C != in.odC || k.D != in.odD || k.clean != in.odClean) {
		odCtlCompute (in, sr, k.ctl);
		k.A     = in.odA;
		k.B     = in.odB;
		k.C     = in.odC;
		k.D     = in.odD;
		k.clean = in.odClean;
		k.valid = true;
	}
	c.odIir        = k.ctl.odIir;
	c.odOutput     = k.ctl.odOutput;
	c.odWet        = k.ctl.odWet;
	c.odDry        = k.ctl.odDry;
	c.odIter       = k.ctl.odIter;
	c.odOut        = k.ctl.odOut;
	c.odDensityPos = k.ctl.odDensityPos;
	c.odClean      = k.ctl.odClean;
}

/* the effect fields of a control entry, from the instance: the mixdown fields that setters
 * change without a tone-generator step (a step's mixCtl writes the same values), preamp,
 * reverb mix, whirl bypass.  The one-shots (whRevOption, whSet) are the caller's. */
static void effectFields (Instance& in, double sr, tbf_seg_ctl& c)
{
	const TgControl& tg = in.tg;
	c.swellPedalGain    = tg.swellPedalGain;
	c.outputGain        = tg.swellPedalGain * tg.percDrawbarGain;
	c.percEnvGainDecay  = tg.percEnvGainDecay;
	c.percEnvGainReset  = tg.percEnvGainReset;
	c.vibTable          = tg.vibTable;
	c.vibMixed          = tg.vibMixed;
	odCtl (in, sr, c);
	c.rvWet    = in.rvG;
	c.whBypass = (uint32_t)in.whBypass;
}

/* a stepper's sink emptied for a chunk (hostControl); its buffers stay allocated */
static void clearSink (ParStep& o)
{
	o.whs.clear (), o.fulls.clear (), o.ctlInst.clear (), o.dInst.clear ();
	o.act.clear (), o.evs.clear (), o.err.clear ();
	o.nd = o.nMsg = o.nGain = o.gainLocal = 0, o.rc = 0, o.fx = false;
}

/* one block of host control for instance i (the message-queue / active-list / routing
 * part of oscGenerateFragment and the effect setters' per-block constants).  Updates
 * the instance's current control e->hCtl[i] / program e->hProg; returns true when the
 * control the next block renders with changed.  rec: device control (the front end here,
 * the per-wheel part in k_tgctl), nullptr under host control.  Key messages, gain pairs and
 * whirl sets go to the sink o, at offsets within it (rec.msgOff, rec.gainOff, whSet). */
static bool stepControl (tbf_engine* e, uint32_t i, bool& progChanged, tbf_tgc_rec* rec, ParStep& o)
{
	Instance&    in      = e->inst[i];
	tbf_seg_ctl& c       = e->hCtl[i];
	progChanged          = false;
	const bool   tgDirty = in.tg.dirty ();
	if (!tgDirty && !in.progDirty && !in.ctlDirty && in.revOpt < 0)
		return false;
	if (tgDirty && rec) {
		const uint32_t at = o.nMsg, ag = o.nGain;
		o.nMsg += (uint32_t)in.tg.msg.size ();
		o.nGain += 2 * in.tg.gainPairs (); /* the changed drawbar gains: (bus, gain) pairs */
		if (o.msgs.size () < o.nMsg) /* by doubling: a resize on every step is a call and a fill */
			o.msgs.resize (2 * (size_t)o.nMsg);
		if (o.gains.size () < o.nGain)
			o.gains.resize (2 * (size_t)o.nGain);
		in.tg.stepFront (o.msgs.data () + at, at, o.gains.data () + ag, ag, *rec, c);
		in.ctlDirty = true;
		progChanged = true;
	} else if (tgDirty) {
		in.tg.step (in.prog, c);
		in.progDirty = true;
		in.ctlDirty  = true;
	}
	if (rec)
		in.progDirty = false; /* device control: programs come from k_tgctl only */
	if (in.progDirty) {
		/* host control: the program in the instance's first slot, behind its header */
		const size_t    np   = std::min (in.prog.size (), SLOT - 1);
		tbf_prog_entry* slot = e->hProg.data () + PSLOTS * i * SLOT;
		slot[0]              = tbf_prog_entry {};
		slot[0].wheel        = 0xFFFF;
		slot[0].pad          = (uint32_t)np;
		std::copy (in.prog.begin (), in.prog.begin () + (long)np, slot + 1);
		c.prog_off   = (uint32_t)(PSLOTS * i * SLOT);
		c.prog_len   = (uint32_t)np;
		in.progDirty = false;
		progChanged  = true;
	}
	effectFields (in, e->cfg.sample_rate, c);
	c.whRevOption = in.revOpt; /* a one-shot: the next block gets a fresh entry without it */
	in.revOpt     = -1;
	c.whSet       = 0;         /* a one-shot too: the whirl keeps a set until the next one */
	if (in.whDirty) {
		o.whs.push_back (in.whr.cur);
		c.whSet    = (uint32_t)o.whs.size ();
		in.whDirty = false;
	}
	in.ctlDirty = (c.whRevOption >= 0) || c.whSet;
	return true;
}

extern "C" int tbf_debug_render_program (tbf_engine* e, uint32_t i, float* out, uint32_t cap)
{
	if (!e || i >= e->inst.size ())
		return fail (-22, "bad instance");
	if (e->devCtl)
		return fail (-95, "host programs: the per-wheel control runs on the device (TBF_HOST_CONTROL=1 for the host path)");
	const size_t n = e->inst.size ();
	if (e->hCtl.size () < n) { /* a host-only engine never sized the pool */
		e->hCtl.resize (n);
		e->hProg.resize (PERSIST (n));
	}
	/* exactly a render's per-block step under host control.  The first sink takes what it emits
	 * (the next chunk clears it): a whSet left in the entry indexes a list never uploaded, as before */
	bool pc;
	if (e->parStep.empty ())
		e->parStep.resize (1);
	(void)stepControl (e, i, pc, nullptr, e->parStep[0]);
	const std::vector<tbf_prog_entry>& prog = e->inst[i].prog;
	for (uint32_t q = 0; q < prog.size () && q < cap; q++) {
		const tbf_prog_entry& p = prog[q];
		float*                o = out + 9 * q;
		o[0] = p.wheel; o[1] = p.env; o[2] = p.row;
		o[3] = p.sg; o[4] = p.pg; o[5] = p.vg; o[6] = p.nsg; o[7] = p.npg; o[8] = p.nvg;
	}
	return (int)prog.size ();
}

/* Device control: the delta that instance i's step just left in e->hCtl[i], as record
 * rec = hRec[base + o.nd] of the sink's part of the staging; returns its pool entry.
 * A stepped delta (k_tgctl rebuilds its program) gets the program slot of its position, any
 * other plays the program of the delta before it (lastProg; `first`: none yet in this chunk,
 * it keeps the persistent one).  A delta that changes only what a key / drawbar step changes
 * travels as its record (k_tgctl rebuilds the entry from the last full one, lastEmit), any
 * other as a full entry in the sink.  allFull (the serial stepper: its one sink's positions
 * are the staging's): every delta a full entry, written straight there, the staging's hFull. */
static uint32_t emitDelta (tbf_engine* e, const Chunk& ck, uint32_t n, uint32_t i, bool stepped, bool first, uint32_t base,
                           tbf_tgc_rec& rec, ParStep& o, PinnedVec<tbf_seg_ctl>* allFull)
{
	const uint32_t d = base + o.nd++;
	tbf_seg_ctl    c = e->hCtl[i];
	if (stepped) {
		c.prog_off = (uint32_t)(PERSIST (n) + ((size_t)ck.rp * n * TBF_CHUNK + d) * SLOT);
		if (!e->stepped[i]) {
			e->stepped[i] = 1;
			o.ctlInst.push_back (i);
		}
	} else {
		memset (&rec, 0, sizeof (rec));
		if (!first)
			c.prog_off = e->lastProg[i];
	}
	e->lastProg[i] = c.prog_off;
	if (!e->dhas[i]) {
		e->dhas[i] = 1;
		o.dInst.push_back (i);
	}
	if (allFull) {
		allFull->push_back (c);
		rec.full = (uint32_t)allFull->size ();
	} else {
		tbf_seg_ctl tc    = e->lastEmit[i];
		tc.prog_off       = c.prog_off;
		tc.keyCompTarget  = c.keyCompTarget;
		tc.resetPercAtEnd = c.resetPercAtEnd;
		tc.routing        = c.routing;
		if (memcmp (&tc, &c, sizeof (c)) != 0) {
			o.fulls.push_back (c);
			rec.full       = (uint32_t)o.fulls.size ();
			e->lastEmit[i] = c;
		}
	}
	rec.keyCompTarget = c.keyCompTarget;
	rec.flags         = (uint8_t)((rec.flags & ~8u) | (c.resetPercAtEnd ? 8u : 0u));
	rec.oldRouting    = (uint8_t)c.routing;
	e->chg[i]         = 1;
	return n + d;
}

/* The sinks of T instance ranges (range t's records at hRec[t * per * want ..)) into the
 * chunk's staging: the lists concatenated in range order, dSeg the filled record segments
 * to upload, and the sink-local offsets -- msgOff behind flag 0x80, gainOff behind flag 4,
 * full, whSet inside the full entries -- rebased here, exactly once.  One range: plain copies. */
static void mergeSinks (tbf_engine* e, ChunkStaging& cs, unsigned T, uint32_t per, uint32_t want)
{
	std::vector<ParStep>& out = e->parStep;
	struct Base { /* a sink's first message, gain float, whirl set and full entry in the chunk's lists */
		size_t m, g, w, f;
	};
	std::vector<Base> b (T + 1, Base {0, 0, 0, 0});
	for (unsigned t = 0; t < T; t++) {
		const ParStep& o = out[t];
		b[t + 1]         = {b[t].m + o.nMsg, b[t].g + o.nGain, b[t].w + o.whs.size (), b[t].f + o.fulls.size ()};
		if (o.nd)
			e->dSeg.push_back ({t * per * want, o.nd});
	}
	cs.hMsg.resize (b[T].m), cs.hGain.resize (b[T].g), cs.hWh.resize (b[T].w);
	if (b[T].f) /* (the serial stepper's are in hFull already) */
		cs.hFull.resize (b[T].f);
	auto copy = [] (auto* dst, const auto& v, size_t count) {
		if (count)
			memcpy ((void*)dst, v.data (), count * sizeof (v[0]));
	};
	if (b[T].m || b[T].g || b[T].w || b[T].f)
		parallelFor (T, [&] (uint32_t t) {
			ParStep&     o    = out[t];
			const size_t base = (size_t)t * per * want;
			for (size_t d = base; t > 0 && d < base + o.nd; d++) { /* (the first range's bases are 0) */
				tbf_tgc_rec& r = cs.hRec[d];
				if (r.flags & 0x80)
					r.msgOff += (uint32_t)b[t].m;
				if (r.flags & 4)
					r.gainOff += (uint32_t)b[t].g;
				if (r.full)
					r.full += (uint32_t)b[t].f;
			}
			for (tbf_seg_ctl& f : o.fulls)
				if (f.whSet)
					f.whSet += (uint32_t)b[t].w;
			copy (cs.hFull.data () + b[t].f, o.fulls, o.fulls.size ());
			copy (cs.hWh.data () + b[t].w, o.whs, o.whs.size ());
			copy (cs.hMsg.data () + b[t].m, o.msgs, o.nMsg);
			copy (cs.hGain.data () + b[t].g, o.gains, o.nGain);
		});
	for (unsigned t = 0; t < T; t++) {
		for (uint32_t i : out[t].ctlInst)
			cs.hCtlInst.push_back (i);
		for (uint32_t i : out[t].dInst)
			cs.hDInst.push_back (i);
	}
}

/* the instance ranges the threaded passes work by: T ranges of `per` instances (the last
 * may be partial), at least 256 instances a range */
static unsigned instanceRanges (uint32_t n, uint32_t& per)
{
	const unsigned T = std::max (1u, std::min<unsigned> (hostThreads (), (n + 255) / 256));
	per              = (n + T - 1) / T;
	return T;
}

/* A stable counting sort of the events of instance range [i0, i1) by instance: each (f)
 * calls f (instance, item) for the range's events in order (it runs twice); instance i's
 * items land in dst[eo[i - i0] .. eo[i - i0 + 1]), for a sequential per-instance pass. */
template <typename Each, typename Item>
static void sortByInstance (uint32_t i0, uint32_t i1, std::vector<uint32_t>& eo, std::vector<uint32_t>& fill, Each each, Item* dst)
{
	const uint32_t m = i1 > i0 ? i1 - i0 : 0;
	eo.assign ((size_t)m + 1, 0);
	each ([&] (uint32_t inst, const Item&) { eo[inst - i0 + 1]++; });
	for (uint32_t q = 0; q < m; q++)
		eo[q + 1] += eo[q];
	fill.assign (eo.begin (), eo.end () - 1);
	each ([&] (uint32_t inst, const Item& item) { dst[fill[inst - i0]++] = item; });
}

static double msBetween (std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b)
{
	return std::chrono::duration<double, std::milli> (b - a).count ();
}

/* the step loop of one instance: its blocks one after another (so its host state stays in
 * the core's L1 over the chunk), its events es[k .. kEnd) (indices into ev, in order) applied
 * at their blocks, a delta where its control changes, its column of the index table.  Writes
 * only the worker's own: records hRec[base + o.nd ..), column i of hIdx, the per-instance
 * arrays at i, the sink o.  Returns false on an event's error (o.rc, o.err). */
static bool stepInstance (tbf_engine* e, ChunkStaging& cs, const Chunk& ck, uint32_t n, uint32_t i, const tbf_event* ev,
                          const uint32_t* es, uint32_t k, uint32_t kEnd, uint32_t base, ParStep& o)
{
	uint32_t ci = i; /* the instance's pool entry at the current block */
	for (uint32_t len = 0; len < ck.want; len++) {
		for (; k < kEnd && ev[es[k]].block <= ck.b0 + len; k++) {
			if ((o.rc = applyEvent (e, ev[es[k]]))) {
				o.err = tbf_last_error (); /* thread-local: copied here, on the worker */
				return false;
			}
			markActive (e, i);
		}
		if (e->inAct[i]) {
			bool         pc;
			tbf_tgc_rec& rec = cs.hRec[base + o.nd];
			if (!e->dseen[i]) { /* the entry the device holds for i at the chunk start */
				e->dseen[i]    = 1;
				e->lastEmit[i] = e->hCtl[i];
			}
			if (stepControl (e, i, pc, &rec, o))
				ci = emitDelta (e, ck, n, i, pc, ci < n, base, rec, o, nullptr);
			else
				e->inAct[i] = 0;
		}
		cs.hIdx[(size_t)len * n + i] = ci;
	}
	e->curIdx[i] = ci;
	return true;
}

/* Device control: one chunk's host control (events + front-end steps) on host worker
 * threads, one contiguous instance range each.  Instances are independent and each keeps
 * its own events' order, so this equals the serial loop; only where the deltas sit in the
 * pool differs: worker t writes its k-th delta to position (first instance of its range) *
 * want + k of the staging (a range of m instances has at most m * want deltas), so nothing
 * is moved afterwards and the kernels reach the deltas through hIdx; dSeg lists the filled
 * segments for the uploads.  Events are [evBeg, evEnd) of ev (block < b0 + want; programme
 * changes excluded by the caller: randomizeDrawbars writes the shared programme table).
 * Fills hRec, hMsg, hGain, hWh, hFull, hCtlInst, hDInst, hIdx (every row), stepped, dhas,
 * curIdx, chg, actList; not dCtl (host control's: k_tgctl builds the deltas' entries).
 * Worker t writes only records [i0 * want, i0 * want + nd) and hIdx columns [i0, i1) of its
 * range [i0, i1), and its own sink.  want <= TBF_CHUNK: a longer chunk has no active
 * instance and no event (chunkLength), so it is the serial stepper's. */
static int stepChunkParallel (tbf_engine* e, ChunkStaging& cs, Chunk& ck, uint32_t n, const tbf_event* ev)
{
	const uint32_t want = ck.want, evBeg = ck.evBeg, evEnd = ck.evEnd;
	uint32_t       per;
	const unsigned T   = instanceRanges (n, per);
	auto&          out = e->parStep;
	out.resize (T);
	for (uint32_t a : e->actList) /* the active list by range, in order */
		out[a / per].act.push_back (a);
	/* the events by instance range, in order: a parallel counting partition over T segments
	 * of the event list (a serial pass cost ~2 ms at 524k events) */
	{
		const uint32_t        nev = evEnd - evBeg, seg = (nev + T - 1) / T;
		std::vector<uint32_t> cnt ((size_t)T * T, 0);
		parallelFor (T, [&] (uint32_t sgm) {
			const uint32_t k0 = evBeg + std::min (nev, sgm * seg), k1 = evBeg + std::min (nev, (sgm + 1) * seg);
			for (uint32_t k = k0; k < k1; k++)
				cnt[(size_t)sgm * T + ev[k].inst / per]++;
		});
		for (unsigned t = 0; t < T; t++) {
			uint32_t tot = 0;
			for (unsigned sgm = 0; sgm < T; sgm++) {
				const uint32_t c                = cnt[(size_t)sgm * T + t];
				cnt[(size_t)sgm * T + t] = tot; /* the segment's first slot in worker t's list */
				tot += c;
			}
			out[t].evs.resize (tot);
		}
		parallelFor (T, [&] (uint32_t sgm) {
			const uint32_t k0 = evBeg + std::min (nev, sgm * seg), k1 = evBeg + std::min (nev, (sgm + 1) * seg);
			uint32_t*      at = cnt.data () + (size_t)sgm * T;
			for (uint32_t k = k0; k < k1; k++) {
				const uint32_t t = ev[k].inst / per;
				out[t].evs[at[t]++] = k;
			}
		});
	}
	cs.hRec.resize ((size_t)n * want);
	e->lastEmit.resize (n);
	e->lastProg.resize (n);
	e->dseen.assign (n, 0);
	const auto            ph0 = std::chrono::steady_clock::now ();
	std::vector<double>   thMs (T);
	parallelFor (T, [&] (uint32_t t) {
		const auto     th0 = std::chrono::steady_clock::now ();
		ParStep&       o   = out[t];
		const uint32_t i0 = t * per, i1 = std::min (n, i0 + per);
		/* markActive's pushes go to the worker's own list while its loop runs, not to the
		 * engine's: set here, cleared below (o.act itself is rebuilt below) */
		tlAct = &o.act;
		o.esort.resize (o.evs.size ());
		sortByInstance (
		    i0, i1, o.eoff, o.efill,
		    [&] (auto f) {
			    for (uint32_t k : o.evs)
				    f (ev[k].inst, k);
		    },
		    o.esort.data ());
		for (uint32_t i = i0; i < i1; i++)
			if (!stepInstance (e, cs, ck, n, i, ev, o.esort.data (), o.eoff[i - i0], o.eoff[i - i0 + 1], i0 * want, o))
				break;
		o.act.clear (); /* the range's instances still active, in order */
		for (uint32_t i = i0; i < i1; i++)
			if (e->inAct[i])
				o.act.push_back (i);
		tlAct   = nullptr;
		thMs[t] = msBetween (th0, std::chrono::steady_clock::now ());
	});
	const auto ph1 = std::chrono::steady_clock::now ();
	for (unsigned t = 0; t < T; t++)
		if (out[t].rc)
			return fail (out[t].rc, out[t].err); /* on the calling thread: the error text is thread-local */
	mergeSinks (e, cs, T, per, want);
	ck.delta = !cs.hDInst.empty (); /* the instances with any delta */
	e->actList.clear (); /* rebuilt in instance order: the ranges' lists, one after another */
	for (unsigned t = 0; t < T; t++)
		e->actList.insert (e->actList.end (), out[t].act.begin (), out[t].act.end ());
	if (e->dbgPhases) {
		double mx = 0, sum = 0;
		for (double v : thMs) {
			mx = std::max (mx, v);
			sum += v;
		}
		fprintf (stderr, "stepChunkParallel T=%u: step %.3f ms (thread max %.3f, mean %.3f) merge %.3f ms\n", T,
		         msBetween (ph0, ph1), mx, sum / T, msBetween (ph1, std::chrono::steady_clock::now ()));
	}
	ck.evBeg = evEnd;
	ck.len   = want;
	return 0;
}

/* Device front end: a chunk whose events are all notes or front-end parameters (frontParam),
 * over instances whose control is otherwise settled (frontClean), is stepped by k_front on
 * the device (csrc/tbf_ctl.hip): the messages, the stepped blocks, the control records and
 * the index table come from the instances' front-end state at the chunk start and their
 * events.  The host only sorts the events by instance and applies them to its own mirror
 * state (the truth for any later host-stepped chunk): no records, no index table. */
static bool frontClean (const Instance& in)
{
	const TgControl& t = in.tg;
	return !in.ctlDirty && !in.progDirty && in.revOpt < 0 && !in.whDirty && t.msg.empty () && !t.drawBarChange &&
	       t.oldRouting == t.newRouting && t.gainsSent && t.gainMask == 0 &&
	       /* the rotary option a drum / horn event derives stays an exact small integer */
	       fabs (in.params[TBF_P_DRUM]) < 1e6 && fabs (in.params[TBF_P_HORN]) < 1e6;
}

/* the instances' front-end cleanliness (e->fclean), once per chunk; false when an active
 * instance is not clean (its pending step is the host's) */
static bool frontCleanAll (tbf_engine* e)
{
	const uint32_t        n  = (uint32_t)e->inst.size ();
	std::vector<uint8_t>& cl = e->fclean;
	cl.resize (n);
	uint32_t       per;
	const unsigned T = instanceRanges (n, per);
	parallelFor (T, [&] (uint32_t t) {
		for (uint32_t i = t * per; i < std::min (n, (t + 1) * per); i++)
			cl[i] = frontClean (e->inst[i]) ? 1 : 0;
	});
	return std::all_of (e->actList.begin (), e->actList.end (), [&] (uint32_t i) { return cl[i] != 0; });
}

/* One parallel pass over a chunk's events (sorted by block): a programme event among them,
 * an event for a bad instance, and -- with cl, the instances' cleanliness -- whether the
 * device front end takes them all (notes and frontParam kinds on clean instances), with
 * the events as compact records bucketed by (segment, instance range) for stepChunkFront.
 * (The records drop the event kind and narrow the value to float: the front end's only.)
 * (Three passes over the 24-B events used to do this: ~0.2 ms each at 524 k events; then a
 * scan, a partition and a gather by instance, ~0.3 ms each.) */
static void scanChunk (uint32_t n, uint32_t b0, const tbf_event* ev, uint32_t evBeg, uint32_t evEnd, const uint8_t* cl,
                       bool& progEv, bool& bad, bool& front, ChunkScan& cs)
{
	const uint32_t nev = evEnd - evBeg;
	cs.T = instanceRanges (n, cs.per);
	assert (cs.T <= TBF_MAX_HOST_THREADS);
	cs.Te  = std::max (1u, std::min (hostThreads (), (nev + 32767) / 32768));
	cs.seg = (nev + cs.Te - 1) / cs.Te;
	if (cl) {
		cs.rec.resize (std::max<uint32_t> (nev, 1));
		cs.boff.resize ((size_t)cs.Te * (cs.T + 1));
	}
	std::vector<char> pe (cs.Te, 0), bd (cs.Te, 0), fr (cs.Te, 0);
	parallelFor (cs.Te, [&] (uint32_t sgm) {
		const uint32_t k0 = evBeg + std::min (nev, sgm * cs.seg), k1 = evBeg + std::min (nev, (sgm + 1) * cs.seg);
		bool           p = false, b = false, f = cl != nullptr; /* locals: the flags share a cache line */
		uint32_t       c[TBF_MAX_HOST_THREADS + 1] = {};         /* events per instance range (T <= TBF_MAX_HOST_THREADS) */
		for (uint32_t k = k0; k < k1; k++) {
			const tbf_event& E = ev[k];
			p                  = p || E.kind == TBF_EV_PROGRAM;
			if (E.inst >= n) {
				b = true;
				f = false;
				continue;
			}
			if (f) {
				f = (E.kind == TBF_EV_NOTE || (E.kind == TBF_EV_PARAM && frontParam (E.id, (float)E.value))) && cl[E.inst];
				c[E.inst / cs.per]++;
			}
		}
		if (f) { /* the records, by range, into this segment's own part of rec (no shared lines) */
			uint32_t* bo = cs.boff.data () + (size_t)sgm * (cs.T + 1);
			uint32_t  at[TBF_MAX_HOST_THREADS];
			bo[0] = k0 - evBeg;
			for (unsigned t = 0; t < cs.T; t++) {
				at[t]     = bo[t];
				bo[t + 1] = bo[t] + c[t];
			}
			ChunkScan::Rec* rec = cs.rec.data ();
			for (uint32_t k = k0; k < k1; k++) {
				const tbf_event& E = ev[k];
				rec[at[E.inst / cs.per]++] = {E.inst, (E.block - b0) << 2 | (E.kind == TBF_EV_PARAM ? 1u : 0u) |
				                                          (E.value != 0.0 ? 2u : 0u),
				                              E.id, (float)E.value};
			}
		}
		pe[sgm] = p;
		bd[sgm] = b;
		fr[sgm] = f;
	});
	progEv = bad = false;
	front        = cl != nullptr;
	for (unsigned t = 0; t < cs.Te; t++) {
		progEv = progEv || pe[t];
		bad    = bad || bd[t];
		front  = front && fr[t];
	}
}

/* an instance's front-end state at the chunk start, as k_front takes it (gainOff: the
 * instance's gain-pair slots within its range; the range's base is added afterwards) */
static void frontSnapshot (const TgControl& tg, uint32_t gainOff, tbf_front_state& F)
{
	memset (&F, 0, sizeof (F));
	static_assert (sizeof (F.keys) == sizeof (tg.keyBits), "384 key bits");
	memcpy (F.keys, tg.keyBits, sizeof (F.keys));
	F.keyDown         = tg.keyDownCount;
	F.upperDown       = (int32_t)tg.upperKeyCount;
	F.pending         = tg.steadyPending ? 1u : 0u;
	F.percSendBus     = tg.percSendBus;
	F.routing         = tg.oldRouting;
	F.percEnabled     = tg.percEnabled ? 1 : 0;
	F.percTrigRestore = tg.percTrigRestore;
	F.percTriggerBus  = tg.percTriggerBus;
	F.percSendBusA    = tg.percSendBusA;
	F.percSendBusB    = tg.percSendBusB;
	F.gainOff         = gainOff;
	F.percReset[0]    = tg.percEnvScaling * tg.percEnvGainResetNorm; /* as setPercVolume */
	F.percReset[1]    = tg.percEnvScaling * tg.percEnvGainResetSoft;
	F.percDrawbar[0]  = tg.percDrawbarNormalGain;
	F.percDrawbar[1]  = tg.percDrawbarSoftGain;
	F.percDecay[0]    = tg.percEnvGainDecaySlowNorm;
	F.percDecay[1]    = tg.percEnvGainDecaySlowSoft;
	F.percDecay[2]    = tg.percEnvGainDecayFastNorm;
	F.percDecay[3]    = tg.percEnvGainDecayFastSoft;
	F.percSoft        = tg.percIsSoft != 0;
	F.percFast        = tg.percIsFast != 0;
	F.swell           = tg.swellPedalGain;
}

/* The mirror of one instance's events es[j0 .. j1) of a front-end chunk (in order; their
 * words go to hFev / hFevVal at wb + j): the host's front state takes them too, through the
 * host path's setter (setParam), with the steps k_front takes -- a block with inputs steps,
 * and so does the one after it; steadyPending and inAct follow from that.  The device writes
 * the chunk's entries; the instance's current entry e->hCtl[i] gets what it ends the chunk with. */
static void mirrorInstance (tbf_engine* e, ChunkStaging& cs, const Chunk& ck, uint32_t i, const ChunkScan::Rec* es,
                            uint32_t j0, uint32_t j1, uint32_t wb, ParStep& o)
{
	Instance&  in      = e->inst[i];
	TgControl& tg      = in.tg;
	bool       stepped = tg.steadyPending, pend = tg.steadyPending, fxd = false;
	uint32_t   oldR = tg.oldRouting, ng = 0, msgsB = 0;
	int        curB = -1;
	auto       closeBlock = [&] () {
        const bool rcp = tg.newRouting != oldR, inputs = msgsB > 0 || tg.drawBarChange || rcp;
        ng += (uint32_t)__builtin_popcount (tg.gainMask);
        stepped = stepped || inputs;
        pend    = inputs;
        oldR    = tg.newRouting;
        tg.drawBarChange = 0;
        tg.gainMask      = 0;
        msgsB            = 0;
	};
	for (uint32_t j = j0; j < j1; j++) {
		const auto&    E   = es[j];
		const uint32_t blk = E.bf >> 2;
		if ((int)blk != curB) {
			if (curB >= 0)
				closeBlock ();
			if (curB >= 0 ? blk > (uint32_t)curB + 1 : blk > 0)
				pend = false; /* blocks without events between: the pending step is done */
			curB = (int)blk;
		}
		if (E.bf & 1u) { /* a parameter: the setter on the mirror, and for an effect the value k_front applies */
			const uint32_t w = frontParam (E.id, E.v);
			cs.hFev[wb + j]  = w | (blk << 16);
			setParam (in, E.id, E.v);
			if (((w >> 12) & 7u) == TBF_FEV_EFFECT) {
				cs.hFevVal[wb + j] = paramRow (E.id)->sent (in, E.v);
				fxd                = true;
			}
			continue;
		}
		const bool on = (E.bf & 2u) != 0;
		const bool ok = E.id >= 0 && E.id < 384; /* oscKeyOn/Off ignore keys >= MAX_KEYS */
		cs.hFev[wb + j] = (ok ? (uint32_t)E.id : 0x0fffu) | (on ? 1u << 12 : 0u) | (blk << 16);
		msgsB += ok ? (uint32_t)tg.noteCount (E.id, on) : 0u;
	}
	if (curB >= 0) {
		closeBlock ();
		if ((uint32_t)curB + 1 < ck.want)
			pend = false;
	} else
		pend = false; /* no events: block 0 takes the pending step */
	o.gainLocal += 2 * ng;
	tg.oldRouting = tg.newRouting;
	tbf_seg_ctl& c = e->hCtl[i];
	if (fxd) {
		/* the rotary option was a one-shot; no step is left pending (setCharacter raised ctlDirty) */
		effectFields (in, e->cfg.sample_rate, c);
		c.whRevOption = -1;
		c.whSet       = 0;
		in.revOpt     = -1;
		in.ctlDirty   = false;
		e->chg[i]     = 1;
		o.fx          = true;
	}
	if (stepped) { /* stepped blocks: control deltas */
		e->stepped[i] = 1;
		o.ctlInst.push_back (i);
		e->chg[i]        = 1;
		const int kd     = tg.keyDownCount;
		c.keyCompTarget  = tg.tpl->keyCompTable[kd < 0 ? 0 : (kd > 127 ? 127 : kd)];
		c.resetPercAtEnd = tg.upperKeyCount == 0;
		c.routing        = tg.oldRouting;
	}
	tg.steadyPending = pend;
	e->inAct[i]      = pend ? 1 : 0;
	if (pend)
		o.act.push_back (i);
}

static int stepChunkFront (tbf_engine* e, ChunkStaging& cs, Chunk& ck, uint32_t n)
{
	const ChunkScan& sc = e->scan; /* the chunk's events, bucketed by scanChunk */
	const unsigned T   = sc.T;
	const uint32_t per = sc.per;
	auto&          out = e->parStep;
	const auto     f0  = std::chrono::steady_clock::now ();
	out.resize (T);
	/* the events by instance range come from scanChunk's buckets, in event order */
	const auto            f1 = std::chrono::steady_clock::now ();
	std::vector<uint32_t> wbase (T + 1, 0);
	auto seg = [&] (unsigned sgm, unsigned t) { return sc.boff.data () + (size_t)sgm * (T + 1) + t; };
	for (unsigned t = 0; t < T; t++) {
		size_t c = 0;
		for (unsigned sgm = 0; sgm < sc.Te; sgm++)
			c += seg (sgm, t)[1] - seg (sgm, t)[0];
		wbase[t + 1] = wbase[t] + (uint32_t)c;
	}
	cs.hFevOff.resize (n + 1);
	cs.hFev.resize (std::max<uint32_t> (wbase[T], 1));
	cs.hFevVal.resize (std::max<uint32_t> (wbase[T], 1));
	cs.hFront.resize (n);
	const bool          dbgPh = e->dbgPhases;
	std::vector<double> thMs (dbgPh ? 3 * T : 0);
	parallelFor (T, [&] (uint32_t t) {
		const auto     g0 = std::chrono::steady_clock::now ();
		ParStep&       o  = out[t];
		const uint32_t i0 = t * per, i1 = std::min (n, i0 + per);
		o.erec.resize (wbase[t + 1] - wbase[t]);
		sortByInstance (
		    i0, i1, o.eoff, o.efill,
		    [&] (auto f) { /* the range's buckets, read in order */
			    for (unsigned sgm = 0; sgm < sc.Te; sgm++)
				    for (uint32_t k = seg (sgm, t)[0]; k < seg (sgm, t)[1]; k++)
					    f (sc.rec[k].inst, sc.rec[k]);
		    },
		    o.erec.data ());
		const auto g1 = std::chrono::steady_clock::now ();
		for (uint32_t i = i0; i < i1; i++) {
			frontSnapshot (e->inst[i].tg, o.gainLocal, cs.hFront[i]);
			cs.hFevOff[i] = wbase[t] + o.eoff[i - i0];
			mirrorInstance (e, cs, ck, i, o.erec.data (), o.eoff[i - i0], o.eoff[i - i0 + 1], wbase[t], o);
		}
		if (dbgPh) {
			const auto g2 = std::chrono::steady_clock::now ();
			thMs[3 * t]     = msBetween (f1, g0); /* start delay */
			thMs[3 * t + 1] = msBetween (g0, g1); /* sort */
			thMs[3 * t + 2] = msBetween (g1, g2); /* mirror */
		}
	});
	cs.hFevOff[n] = wbase[T];
	{ /* the gain-pair slots: each range's base */
		std::vector<uint32_t> gb (T + 1, 0);
		for (unsigned t = 0; t < T; t++)
			gb[t + 1] = gb[t] + out[t].gainLocal;
		e->frontGain = gb[T];
		parallelFor (T, [&] (uint32_t t) {
			for (uint32_t i = t * per; i < std::min (n, (t + 1) * per); i++)
				cs.hFront[i].gainOff += gb[t];
		});
	}
	e->actList.clear (); /* rebuilt in instance order */
	for (unsigned t = 0; t < T; t++) {
		e->actList.insert (e->actList.end (), out[t].act.begin (), out[t].act.end ());
		for (uint32_t i : out[t].ctlInst)
			cs.hCtlInst.push_back (i);
		ck.delta = ck.delta || out[t].fx || !out[t].ctlInst.empty ();
	}
	if (dbgPh) {
		fprintf (stderr, "stepChunkFront T=%u: partition %.3f ms, instances %.3f ms\n", T, msBetween (f0, f1),
		         msBetween (f1, std::chrono::steady_clock::now ()));
		double mx[3] = {0, 0, 0}, sm[3] = {0, 0, 0};
		for (unsigned t = 0; t < T; t++)
			for (int q = 0; q < 3; q++) {
				mx[q] = std::max (mx[q], thMs[3 * t + q]);
				sm[q] += thMs[3 * t + q] / T;
			}
		fprintf (stderr, "  threads (mean / max ms): start %.3f / %.3f, sort %.3f / %.3f, mirror %.3f / %.3f\n", sm[0], mx[0],
		         sm[1], mx[1], sm[2], mx[2]);
	}
	ck.evBeg = ck.evEnd;
	ck.len   = ck.want;
	return 0;
}

/* The serial host control step, block by block: entry indices per (block, instance), new
 * pool entries only where an instance's control changes.  Host control's one path (the
 * deltas' entries in dCtl, their programs in dProg); device control's for few active
 * instances or a programme event (every delta a full entry).  One sink, one range at base 0.
 * May end the chunk early -- delta programs full (host control), or TBF_CHUNK blocks reached
 * with a delta: no delta chunk is longer -- and leaves ck.evBeg behind the events applied. */
static int stepChunkSerial (tbf_engine* e, ChunkStaging& cs, Chunk& ck, uint32_t n, const tbf_event* ev)
{
	std::vector<uint32_t>& cur = e->curIdx;
	uint32_t&              len = ck.len;
	ParStep&               o   = e->parStep[0];
	if (e->devCtl) /* emitDelta keeps the last delta's program there, as for the threaded stepper */
		e->lastProg.resize (n);
	for (; len < ck.want; len++) {
		if (!e->devCtl && e->dProg.size () + (size_t)n * SLOT > DPROG_CAP (n) && len > 0)
			break; /* delta program pool full: end the chunk here */
		if (ck.delta && len >= TBF_CHUNK)
			break; /* a chunk with deltas ends at TBF_CHUNK blocks, before the next block's events */
		for (; ck.evBeg < ck.evEnd && ev[ck.evBeg].block <= ck.b0 + len; ck.evBeg++) {
			if (int rc = applyEvent (e, ev[ck.evBeg]))
				return rc;
			markActive (e, ev[ck.evBeg].inst);
		}
		if (e->devCtl) /* room for a record from every active instance */
			cs.hRec.resize ((size_t)o.nd + e->actList.size ());
		/* only the instances whose control may still change are stepped: one that
		 * steps to no change stays unchanged until an event touches it */
		const bool hadDelta = ck.delta;
		size_t     keep     = 0;
		for (size_t a = 0; a < e->actList.size (); a++) {
			const uint32_t i = e->actList[a];
			bool           pc;
			tbf_tgc_rec*   rec = e->devCtl ? &cs.hRec[o.nd] : nullptr;
			if (!stepControl (e, i, pc, rec, o)) {
				e->inAct[i] = 0;
				continue;
			}
			if (e->devCtl)
				cur[i] = emitDelta (e, ck, n, i, pc, cur[i] < n, 0, *rec, o, &cs.hFull);
			else {
				tbf_seg_ctl c = e->hCtl[i];
				if (pc) {
					c.prog_off = (uint32_t)(PERSIST (n) + e->dProg.size ());
					e->dProg.insert (e->dProg.end (), e->hProg.begin () + PSLOTS * i * SLOT,
					                 e->hProg.begin () + PSLOTS * i * SLOT + 1 + c.prog_len);
				} else if (cur[i] >= n)
					c.prog_off = cs.dCtl[cur[i] - n].prog_off; /* program of the previous delta */
				cur[i] = n + (uint32_t)cs.dCtl.size ();
				cs.dCtl.push_back (c);
				e->chg[i] = 1;
			}
			ck.delta           = true;
			e->actList[keep++] = i;
		}
		e->actList.resize (keep);
		/* entry index table: written only once the chunk has a delta (before that
		 * every row is the identity) */
		if (ck.delta) {
			if (!hadDelta)
				for (uint32_t r = 0; r < len; r++)
					for (uint32_t i = 0; i < n; i++)
						cs.hIdx[(size_t)r * n + i] = i;
			std::copy (cur.begin (), cur.end (), cs.hIdx.begin () + (size_t)len * n);
		}
	}
	cs.hRec.resize (o.nd);
	mergeSinks (e, cs, 1, n, ck.want);
	return 0;
}

/* The chunk's host control: its events [evBeg, evEnd) found and checked, then stepped by
 * one of stepChunkFront, stepChunkParallel and stepChunkSerial into a cleared staging set.
 * Leaves ck.len, ck.delta, ck.dfront, ck.evBeg behind the events applied, and in dSeg the
 * segments of hRec to upload (none for a front-end chunk: k_front writes the records). */
int tbf::hostControl (tbf_engine* e, ChunkStaging& cs, Chunk& ck, uint32_t n, const tbf_event* ev, uint32_t nev)
{
	const uint32_t b0 = ck.b0, want = ck.want, evi = ck.evBeg;
	cs.dCtl.clear (), cs.hRec.clear (), cs.hMsg.clear (), cs.hGain.clear (), cs.hWh.clear ();
	cs.hCtlInst.clear (), cs.hDInst.clear (), cs.hFull.clear ();
	e->dSeg.clear (), e->dProg.clear ();
	e->stepped.assign (n, 0), e->dhas.assign (n, 0);
	cs.hIdx.resize ((size_t)want * n);
	e->curIdx.resize (n);
	for (uint32_t i = 0; i < n; i++)
		e->curIdx[i] = i;
	const auto hc0 = std::chrono::steady_clock::now ();
	e->parStep.resize (std::max<size_t> (e->parStep.size (), 1)); /* the steppers' sinks, emptied */
	for (ParStep& o : e->parStep)
		clearSink (o);
	/* the chunk's events (sorted by block: a binary search), checked in parallel (a serial
	 * pass cost ~0.5 ms at 524k events) */
	const uint32_t evEnd = ck.evEnd = (uint32_t)(
	    std::partition_point (ev + evi, ev + nev, [&] (const tbf_event& x) { return x.block < b0 + want; }) - ev);
	/* a chunk of note, drawbar and switch events only (frontParam) on clean instances: the
	 * device front end */
	bool       progEv = false, badEv = false, front = false;
	const bool frontCand = e->devCtl && ck.dpipe && e->frontOn && evEnd - evi >= e->frontMin && frontCleanAll (e);
	const auto sc0       = std::chrono::steady_clock::now ();
	scanChunk (n, b0, ev, evi, evEnd, frontCand ? e->fclean.data () : nullptr, progEv, badEv, front, e->scan);
	if (e->dbgPhases)
		fprintf (stderr, "chunk %llu: clean %.3f ms, scan %.3f ms (%u events)\n", (unsigned long long)e->chunkSeq,
		         msBetween (hc0, sc0), msBetween (sc0, std::chrono::steady_clock::now ()), evEnd - evi);
	if (badEv)
		return fail (-22, "event for a bad instance");
	int rc;
	if (frontCand && front && !progEv) {
		if ((rc = stepChunkFront (e, cs, ck, n)))
			return rc;
		ck.dfront = true;
		e->frontChunks[0]++;
		if (e->dbgPhases)
			fprintf (stderr, "chunk %llu: device front end, %u note events\n", (unsigned long long)e->chunkSeq,
			         cs.hFevOff[n]);
	} else {
		if (evEnd > evi)
			e->frontChunks[1]++;
		/* device control with many instances to step (active now, or touched by this chunk's
		 * events): the chunk's host control on worker threads (serial when a programme change
		 * is among the events) */
		if (e->devCtl && !progEv && e->parCtl && e->actList.size () + (evEnd - evi) >= 1024)
			rc = stepChunkParallel (e, cs, ck, n, ev);
		else
			rc = stepChunkSerial (e, cs, ck, n, ev);
		if (rc)
			return rc;
	}
	e->hostCtlNs += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds> (
	                    std::chrono::steady_clock::now () - hc0)
	                    .count ();
	e->hostCtlBlocks += ck.len;
	if (ck.delta && ck.len > TBF_CHUNK)
		return fail (-5, "internal: a chunk with control deltas longer than 64 blocks");
	return 0;
}
