/*
 * tbf_fork.cpp -- tbf_instances_clone / tbf_instances_save / tbf_instances_load: an
 * instance's complete state captured and installed in another slot.
 *
 * One capture / install pair serves the three calls.  The rule is copy, never re-derive:
 * stepping the control plane again for the new slot would not reproduce the envelope
 * entries in flight, steadyPending or the persistent-slot rotation.  The only fields that
 * change are those that encode the slot's position (the prog_off of hCtl / lastEmit and
 * lastProg), which move by the distance between the slots' persistent program ranges.
 *   host part    the whole Instance, field by field (ioInstance / ioTg: the vectors by
 *                length and content, the template pointer from its id), hCtl, the instance's
 *                slots of hProg, pslot, lastEmit, lastProg, membership in `retuned`
 *   device part  st, wring, rslab, tgc (device control) and the persistent program slots,
 *                moved by k_state_move (csrc/tbf_state.hip): array to array for a clone, to
 *                and from one packed record per instance for a save / load
 * A blob is the header, one directory entry per instance, the host records, then the device
 * records; the header carries a checksum of everything behind it, and every offset and
 * length is re-derived and compared on load, so a blob that was cut or altered is refused
 * before anything is touched.
 * tbf_instances_remove (at the end) moves the same parts of every survivor, with the same
 * mover and the same rebase, into arrays sized for the new count.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_engine_impl.h"
#include "tbf_state.h"

extern "C" int tbf_launch_state_move (tbf_move_table* T, const uint32_t* dPairSrc, const uint32_t* dPairDst,
                                      uint32_t npairs, uint32_t unroll, hipStream_t stream);

using namespace tbf;

static_assert (sizeof (tbf_inst_state) % 8 == 0, "k_state_move's narrow path moves 8-B elements");
static_assert (sizeof (tbf_tgc_state) % 16 == 0 && sizeof (tbf_prog_entry) % 16 == 0, "16-B segments");

namespace {

/* ------------------------------------------------------------------ fingerprints */

/* a 64-bit multiplicative hash over 4-byte words (the tables are float / uint32 arrays) */
struct Hash {
	uint64_t h = 0xcbf29ce484222325ull;
	void     words (const void* p, size_t bytes)
	{
		const unsigned char* b = (const unsigned char*)p;
		for (size_t i = 0; i + 4 <= bytes; i += 4) {
			uint32_t w;
			memcpy (&w, b + i, 4);
			h = (h ^ w) * 0x100000001b3ull;
			h ^= h >> 29;
		}
	}
};

/* the checksum of a blob's body: four independent 64-bit lanes over 32-byte groups (a blob of
 * 4096 instances is 1.4 GB: one dependent multiply per word would take longer than its copy) */
uint64_t bodyHash (const unsigned char* p, uint64_t bytes)
{
	uint64_t h[4] = {0x9e3779b97f4a7c15ull, 0xbf58476d1ce4e5b9ull, 0x94d049bb133111ebull, 0xcbf29ce484222325ull};
	uint64_t i    = 0;
	for (; i + 32 <= bytes; i += 32) {
		uint64_t w[4];
		memcpy (w, p + i, 32);
		for (int q = 0; q < 4; q++) {
			h[q] = (h[q] ^ w[q]) * 0x100000001b3ull;
			h[q] ^= h[q] >> 31;
		}
	}
	uint64_t t[4] = {0, 0, 0, 0};
	memcpy (t, p + i, bytes - i);
	uint64_t r = bytes;
	for (int q = 0; q < 4; q++) {
		r = (r ^ h[q] ^ t[q]) * 0xff51afd7ed558ccdull;
		r ^= r >> 33;
	}
	return r;
}

/* the engine-wide tables a cfg shapes: whirl displacement / bw tables, scanner tables,
 * stator increment */
uint64_t engineFingerprint (tbf_engine* e)
{
	if (!e->engFp) {
		Hash H;
		H.words (e->wt.displ.data (), e->wt.displ.size () * sizeof (float));
		H.words (e->wt.bw.data (), e->wt.bw.size () * sizeof (float));
		H.words (e->vibTab.data (), e->vibTab.size () * sizeof (uint32_t));
		H.words (&e->statorInc, sizeof (e->statorInc));
		e->engFp = H.h | 1u; /* 0 stands for "not computed" */
	}
	return e->engFp;
}

/* a template's tables: wave lengths, bank, both envelope tables, key compression */
uint64_t templateFingerprint (tbf_engine* e, uint32_t id)
{
	if (e->tplFp.size () < e->tpls.size ())
		e->tplFp.resize (e->tpls.size (), 0);
	if (!e->tplFp[id]) {
		const TgTemplate& t = *e->tpls[id];
		Hash              H;
		H.words (t.len, sizeof (t.len));
		H.words (t.bank.data (), t.bank.size () * sizeof (float));
		H.words (t.attackEnv, sizeof (t.attackEnv));
		H.words (t.releaseEnv, sizeof (t.releaseEnv));
		H.words (t.keyCompTable, sizeof (t.keyCompTable));
		e->tplFp[id] = H.h | 1u;
	}
	return e->tplFp[id];
}

/* ------------------------------------------------------------------ host records */

/* writes into [p, p + cap) (p NULL: counts only) */
struct Writer {
	unsigned char* p   = nullptr;
	uint64_t       cap = 0, at = 0;
	bool           ok  = true;
	void raw (const void* src, uint64_t len)
	{
		if (p) {
			if (len > cap - std::min (at, cap))
				ok = false;
			else if (len)
				memcpy (p + at, src, len);
		}
		at += len;
	}
	template <typename T>
	void pod (T& v)
	{
		static_assert (std::is_trivially_copyable<T>::value, "pod");
		raw (&v, sizeof (T));
	}
	template <typename T>
	void vec (std::vector<T>& v, uint64_t)
	{
		static_assert (std::is_trivially_copyable<T>::value, "vec");
		uint64_t n = v.size ();
		raw (&n, sizeof (n));
		raw (v.data (), n * sizeof (T));
	}
	void align (uint64_t a)
	{
		static const unsigned char zero[16] = {0};
		while (at % a)
			raw (zero, std::min<uint64_t> (a - at % a, sizeof (zero)));
	}
};

/* reads from [p, p + size): every length is checked against what is left */
struct Reader {
	const unsigned char* p    = nullptr;
	uint64_t             size = 0, at = 0;
	bool                 ok   = true;
	void raw (void* dst, uint64_t len)
	{
		if (!ok || len > size - std::min (at, size)) {
			ok = false;
			return;
		}
		if (len)
			memcpy (dst, p + at, len);
		at += len;
	}
	template <typename T>
	void pod (T& v)
	{
		static_assert (std::is_trivially_copyable<T>::value, "pod");
		raw (&v, sizeof (T));
	}
	template <typename T>
	void vec (std::vector<T>& v, uint64_t maxCount)
	{
		uint64_t n = 0;
		raw (&n, sizeof (n));
		if (!ok || n > maxCount || n * sizeof (T) > size - at) {
			ok = false;
			return;
		}
		v.resize ((size_t)n);
		raw (v.data (), n * sizeof (T));
	}
	void align (uint64_t a) { at = (at + a - 1) / a * a; }
};

/* TgControl, member by member (the template pointer comes from the instance's id) */
template <typename A>
void ioTg (A& a, TgControl& t)
{
	a.vec (t.wh, 1);
	a.vec (t.msg, 1u << 24);
	a.pod (t.keyDownCount);
	a.pod (t.upperKeyCount);
	a.pod (t.newRouting);
	a.pod (t.oldRouting);
	a.pod (t.percSendBus);
	a.pod (t.percSendBusA);
	a.pod (t.percSendBusB);
	a.pod (t.swellPedalGain);
	a.pod (t.outputLevelTrim);
	a.pod (t.keyBits);
	a.pod (t.drawBarGain);
	a.pod (t.drawBarLevel);
	a.pod (t.drawBarChange);
	a.pod (t.percEnabled);
	a.pod (t.percTriggerBus);
	a.pod (t.percTrigRestore);
	a.pod (t.percIsSoft);
	a.pod (t.percIsFast);
	a.pod (t.percEnvGainReset);
	a.pod (t.percEnvGainDecay);
	a.pod (t.percEnvScaling);
	a.pod (t.percEnvGainResetNorm);
	a.pod (t.percEnvGainResetSoft);
	a.pod (t.percEnvGainDecayFastNorm);
	a.pod (t.percEnvGainDecayFastSoft);
	a.pod (t.percEnvGainDecaySlowNorm);
	a.pod (t.percEnvGainDecaySlowSoft);
	a.pod (t.percDrawbarNormalGain);
	a.pod (t.percDrawbarSoftGain);
	a.pod (t.percDrawbarGain);
	a.pod (t.vibTable);
	a.pod (t.vibMixed);
	a.pod (t.steadyPending);
	a.pod (t.gainsSent);
	a.pod (t.gainMask);
}

template <typename A>
void ioInstance (A& a, Instance& in)
{
	a.pod (in.tpl);
	ioTg (a, in.tg);
	a.pod (in.k);
	a.pod (in.s0);
	a.pod (in.ctl);
	a.pod (in.params);
	a.pod (in.odClean);
	a.pod (in.odA);
	a.pod (in.odB);
	a.pod (in.odC);
	a.pod (in.odD);
	a.pod (in.odc);
	a.pod (in.rvG);
	a.pod (in.cabWet);
	a.pod (in.rsPos);
	a.pod (in.whBypass);
	a.pod (in.revOpt);
	a.pod (in.revSelect);
	a.pod (in.whr);
	a.pod (in.whDirty);
	a.pod (in.ctlRand);
	a.pod (in.ctlDirty);
	a.pod (in.progDirty);
	a.vec (in.prog, 1u << 20);
}

/* what the engine keeps per instance outside Instance.  The program offsets are stored
 * relative to the slot's own persistent range, so they land on the destination's */
struct SlotRec {
	uint32_t                    has = 0; /* 1: hCtl / hProg / pslot, 2: lastEmit, 4: lastProg, 8: in `retuned` */
	uint32_t                    pslot = 0;
	tbf_seg_ctl                 ctl = {}, lastEmit = {};
	uint32_t                    lastProg = 0, pad = 0;
	std::vector<tbf_prog_entry> prog; /* PSLOTS * SLOT entries */
};

template <typename A>
void ioSlot (A& a, SlotRec& s)
{
	a.pod (s.has);
	a.pod (s.pslot);
	a.pod (s.ctl);
	a.pod (s.lastEmit);
	a.pod (s.lastProg);
	a.pod (s.pad);
	a.vec (s.prog, PSLOTS * SLOT);
}

uint32_t progBase (uint32_t i) { return (uint32_t)(PSLOTS * i * SLOT); }

bool inRetuned (const tbf_engine* e, uint32_t i)
{
	return std::find (e->retuned.begin (), e->retuned.end (), i) != e->retuned.end ();
}

/* capture: instance i's engine-side record (withProg false: without its slots of hProg,
 * which a clone copies inside hProg itself, 25 KB per instance) */
void captureSlot (const tbf_engine* e, uint32_t i, SlotRec& s, bool withProg = true)
{
	s = SlotRec ();
	if (i < e->hCtl.size () && PERSIST (i + 1) <= e->hProg.size () && i < e->pslot.size ()) {
		s.has |= 1u;
		s.ctl = e->hCtl[i];
		s.ctl.prog_off -= progBase (i);
		s.pslot = e->pslot[i];
		if (withProg)
			s.prog.assign (e->hProg.begin () + (long)PERSIST (i), e->hProg.begin () + (long)PERSIST (i + 1));
	}
	if (i < e->lastEmit.size ()) {
		s.has |= 2u;
		s.lastEmit = e->lastEmit[i];
		s.lastEmit.prog_off -= progBase (i);
	}
	if (i < e->lastProg.size ()) {
		s.has |= 4u;
		s.lastProg = e->lastProg[i] - progBase (i);
	}
	if (inRetuned (e, i))
		s.has |= 8u;
}

/* install: the record into slot i (the engine's arrays already reach i where the record
 * has the part; lastEmit / lastProg grow as stepChunkParallel would size them) */
void installSlot (tbf_engine* e, uint32_t i, const SlotRec& s)
{
	const size_t n = e->inst.size ();
	if ((s.has & 1u) && i < e->hCtl.size () && PERSIST (i + 1) <= e->hProg.size () && i < e->pslot.size ()) {
		e->hCtl[i] = s.ctl;
		e->hCtl[i].prog_off += progBase (i);
		e->pslot[i] = (uint8_t)s.pslot;
		if (!s.prog.empty ())
			std::copy (s.prog.begin (), s.prog.end (), e->hProg.begin () + (long)PERSIST (i));
	}
	if (s.has & 2u) {
		if (e->lastEmit.size () < n)
			e->lastEmit.resize (n);
		e->lastEmit[i] = s.lastEmit;
		e->lastEmit[i].prog_off += progBase (i);
	}
	if (s.has & 4u) {
		if (e->lastProg.size () < n)
			e->lastProg.resize (n);
		e->lastProg[i] = s.lastProg + progBase (i);
	}
	const bool was = inRetuned (e, i);
	if ((s.has & 8u) && !was)
		e->retuned.push_back (i);
	else if (!(s.has & 8u) && was)
		e->retuned.erase (std::find (e->retuned.begin (), e->retuned.end (), i));
}

/* a host-only engine sizes its control pool on demand (tbf_debug_render_program): when a
 * record brings pool entries, the pool reaches every instance first */
void hostPool (tbf_engine* e, const std::vector<SlotRec>& recs)
{
	bool any = !e->hCtl.empty ();
	for (const SlotRec& r : recs)
		any = any || (r.has & 1u);
	const size_t n = e->inst.size ();
	if (any && e->hCtl.size () < n) {
		e->hCtl.resize (n);
		e->hProg.resize (PERSIST (n));
		e->pslot.resize (n, 0);
	}
}

/* after an install: every instance is stepped at the next block (one with nothing pending
 * steps to no change) and both control regions and the persistent pool refresh, as after
 * tbf_instances_add */
void afterInstall (tbf_engine* e)
{
	e->actAll       = true;
	e->persistStale = true;
	e->ctlVer++;
}

/* ------------------------------------------------------------------ device records */

uint64_t align16 (uint64_t v) { return (v + 15) & ~(uint64_t)15; }

/* the per-instance device arrays: base, bytes per instance */
struct DevSeg {
	unsigned char* base;
	uint64_t       bytes;
};

uint32_t deviceSegments (const tbf_engine* e, DevSeg* s)
{
	uint32_t n = 0;
	s[n++]     = {(unsigned char*)e->st.p, sizeof (tbf_inst_state)};
	s[n++]     = {(unsigned char*)e->wring.p, (uint64_t)4 * e->wringLen * sizeof (float)};
	s[n++]     = {(unsigned char*)e->rslab.p, (uint64_t)e->slabLen * sizeof (double)};
	if (e->devCtl)
		s[n++] = {(unsigned char*)e->tgc.p, sizeof (tbf_tgc_state)};
	s[n++] = {(unsigned char*)e->prog.p, PSLOTS * SLOT * sizeof (tbf_prog_entry)};
	if (e->cab.K) /* the cabinet convolver's history (csrc/tbf_cabinet.h) */
		s[n++] = {(unsigned char*)e->cab.st.p, e->cab.instFloats () * sizeof (float)};
	if (e->rs.L) /* the rate converter's history (csrc/tbf_resample.h) */
		s[n++] = {(unsigned char*)e->rs.st.p, e->rs.instFloats () * sizeof (float)};
	static_assert (7 <= TBF_MOVE_SEGS, "deviceSegments lists up to seven arrays");
	return n;
}

/* bytes of one packed device record: the segments one after another, each from a 16-B boundary */
uint64_t deviceRecordBytes (const tbf_engine* e)
{
	DevSeg         s[TBF_MOVE_SEGS];
	const uint32_t ns = deviceSegments (e, s);
	uint64_t       o  = 0;
	for (uint32_t g = 0; g < ns; g++)
		o = align16 (o) + s[g].bytes;
	return align16 (o);
}

/* One k_state_move over the pairs (src[k] -> dst[k]).  mode 0: array to array (clone; with
 * `into`, the segments of other arrays in deviceSegments' order, from the engine's arrays into
 * those: a removal's compaction); 1: array to record k of `stage` (save); 2: record k of
 * `stage` to array (load).  For 1 / 2 the record side's index list is 0 .. np - 1.  On the
 * engine's stream; the caller waits. */
int moveState (tbf_engine* e, int mode, const uint32_t* src, const uint32_t* dst, uint32_t np, unsigned char* stage,
               const DevSeg* into = nullptr)
{
	if (np == 0)
		return 0;
	DevSeg         s[TBF_MOVE_SEGS];
	const uint32_t ns  = deviceSegments (e, s);
	const uint64_t rec = deviceRecordBytes (e);
	tbf_move_table T;
	memset (&T, 0, sizeof (T));
	T.nseg     = ns;
	uint64_t o = 0;
	for (uint32_t g = 0; g < ns; g++) {
		o               = align16 (o);
		tbf_move_seg& M = T.seg[g];
		M.bytes         = s[g].bytes;
		M.src           = mode == 2 ? stage + o : s[g].base;
		M.srcStride     = mode == 2 ? rec : s[g].bytes;
		M.dst           = mode == 1 ? stage + o : (mode == 0 && into) ? into[g].base : s[g].base;
		M.dstStride     = mode == 1 ? rec : s[g].bytes;
		/* the width, per segment: 16 B where both bases, both strides and the length allow */
		M.wide = (M.bytes % 16 == 0 && M.srcStride % 16 == 0 && M.dstStride % 16 == 0 && (uintptr_t)M.src % 16 == 0 &&
		          (uintptr_t)M.dst % 16 == 0)
		             ? 1u
		             : 0u;
		o += s[g].bytes;
	}
	if (e->stPairs.cap < 2 * (size_t)np && e->stPairs.ensure (2 * (size_t)np))
		return fail (-12, "out of device memory (state pairs)");
	HIPCHK (hipMemcpy (e->stPairs.p, src, np * sizeof (uint32_t), hipMemcpyHostToDevice));
	HIPCHK (hipMemcpy (e->stPairs.p + np, dst, np * sizeof (uint32_t), hipMemcpyHostToDevice));
	/* four loads per lane in flight when the grid fills the chip either way; one, and four
	 * times the workgroups, for a few pairs */
	const uint64_t big    = (rec + 16383) / 16384 * np;
	const uint32_t unroll = big >= 4 * (uint64_t)e->nCU ? 4u : 1u;
	for (uint32_t k = 0; k < np; k += 32768) {
		const uint32_t m = std::min (np - k, 32768u);
		tbf_move_table Tk = T;
		if (tbf_launch_state_move (&Tk, e->stPairs.p + k, e->stPairs.p + np + k, m, unroll, e->stream))
			return fail (-5, std::string ("k_state_move launch failed: ") + hipGetErrorString (hipGetLastError ()));
	}
	return 0;
}

/* ------------------------------------------------------------------ blob layout */

#define TBF_BLOB_MAGIC 0x3145544154534654ull /* "TFSTATE1" */

struct BlobHdr {
	uint64_t magic;
	uint32_t hdrBytes, count;
	/* sizeof of every dumped struct: a blob is valid for the build that wrote it only */
	uint32_t szInstance, szTgControl, szWheels, szInstState, szInstConst, szSegCtl, szProgEntry, szTgcState, szWhParams,
	    szWhirlRt, szRand, szOdCache;
	double   sampleRate;
	uint32_t chain, device, devCtl, wringLen, slabLen, progSlots;
	uint64_t engineFp;
	uint32_t cabTaps, cabPad;  /* the cabinet response: its length (0: none) and the fingerprint of its taps */
	uint64_t cabFp;
	uint32_t rsFo, rsL, rsM, rsT; /* the rate converter: output rate (0: none), ratio, taps per phase, and the */
	uint64_t rsFp;                /* fingerprint of its table */
	uint64_t devStride;        /* bytes of one device record (0 on a host-only engine) */
	uint64_t hostOff, devOff;  /* the host records, the device records */
	uint64_t bodyHash;         /* checksum of everything behind the header */
	uint64_t total;            /* bytes of the whole blob */
};

struct BlobInst {
	uint32_t tpl, pad;
	uint64_t tplFp;
	uint64_t hostOff, hostLen; /* the instance's host record */
};

void fillHeader (tbf_engine* e, uint32_t n, BlobHdr& h)
{
	memset (&h, 0, sizeof (h));
	h.magic       = TBF_BLOB_MAGIC;
	h.hdrBytes    = sizeof (BlobHdr);
	h.count       = n;
	h.szInstance  = sizeof (Instance);
	h.szTgControl = sizeof (TgControl);
	h.szWheels    = sizeof (TgControl::Wheels);
	h.szInstState = sizeof (tbf_inst_state);
	h.szInstConst = sizeof (tbf_inst_const);
	h.szSegCtl    = sizeof (tbf_seg_ctl);
	h.szProgEntry = sizeof (tbf_prog_entry);
	h.szTgcState  = sizeof (tbf_tgc_state);
	h.szWhParams  = sizeof (tbf_wh_params);
	h.szWhirlRt   = sizeof (WhirlRt);
	h.szRand      = sizeof (GlibcRand);
	h.szOdCache   = sizeof (Instance::OdCache);
	h.sampleRate  = e->cfg.sample_rate;
	h.chain       = e->cfg.chain_mode;
	h.device      = e->cfg.device >= 0 ? 1u : 0u;
	h.devCtl      = e->devCtl ? 1u : 0u;
	h.wringLen    = e->wringLen;
	h.slabLen     = e->slabLen;
	h.progSlots   = (uint32_t)(PSLOTS * SLOT);
	h.engineFp    = engineFingerprint (e);
	h.cabTaps     = e->cab.taps;
	h.cabFp       = e->cab.fp;
	h.rsFo        = e->rs.Fo;
	h.rsL         = e->rs.L;
	h.rsM         = e->rs.M;
	h.rsT         = e->rs.T;
	h.rsFp        = e->rs.fp;
	h.devStride   = h.device ? deviceRecordBytes (e) : 0;
	h.hostOff     = sizeof (BlobHdr) + (uint64_t)n * sizeof (BlobInst);
}

/* the first header field of `b` that differs from what this engine writes, or NULL */
const char* headerMismatch (const BlobHdr& b, const BlobHdr& h)
{
#define FIELD(f, name) \
	if (b.f != h.f)    \
		return name;
	FIELD (magic, "magic (not a state blob)")
	FIELD (hdrBytes, "header size")
	FIELD (szInstance, "sizeof (Instance)")
	FIELD (szTgControl, "sizeof (TgControl)")
	FIELD (szWheels, "sizeof (TgControl::Wheels)")
	FIELD (szInstState, "sizeof (tbf_inst_state)")
	FIELD (szInstConst, "sizeof (tbf_inst_const)")
	FIELD (szSegCtl, "sizeof (tbf_seg_ctl)")
	FIELD (szProgEntry, "sizeof (tbf_prog_entry)")
	FIELD (szTgcState, "sizeof (tbf_tgc_state)")
	FIELD (szWhParams, "sizeof (tbf_wh_params)")
	FIELD (szWhirlRt, "sizeof (WhirlRt)")
	FIELD (szRand, "sizeof (GlibcRand)")
	FIELD (szOdCache, "sizeof (Instance::OdCache)")
	FIELD (sampleRate, "sample rate")
	FIELD (chain, "chain mode")
	FIELD (device, "device / host-only engine")
	FIELD (devCtl, "control path (device / host control)")
	FIELD (wringLen, "whirl ring window (wringLen)")
	FIELD (slabLen, "reverb slab length (slabLen)")
	FIELD (progSlots, "program slots per instance")
	FIELD (engineFp, "engine fingerprint (whirl / scanner tables)")
	FIELD (cabTaps, "cabinet response length (tbf_cabinet_set)")
	FIELD (cabPad, "cabinet header word")
	FIELD (cabFp, "cabinet response taps (tbf_cabinet_set)")
	FIELD (rsFo, "resampler output rate (tbf_resampler_set)")
	FIELD (rsL, "resampler ratio L (tbf_resampler_set)")
	FIELD (rsM, "resampler ratio M (tbf_resampler_set)")
	FIELD (rsT, "resampler taps per phase (tbf_resampler_set)")
	FIELD (rsFp, "resampler table (tbf_resampler_set)")
	FIELD (count, "instance count")
	FIELD (devStride, "device record size")
	FIELD (hostOff, "host record offset")
#undef FIELD
	return nullptr;
}

int checkInstances (const tbf_engine* e, uint32_t n, const uint32_t* inst, bool distinct)
{
	if (!e || (n && !inst))
		return fail (-22, "null argument");
	for (uint32_t k = 0; k < n; k++)
		if (inst[k] >= e->inst.size ())
			return fail (-22, "instance " + std::to_string (inst[k]) + " does not exist");
	if (distinct) {
		std::vector<uint8_t> seen (e->inst.size (), 0);
		for (uint32_t k = 0; k < n; k++) {
			if (seen[inst[k]])
				return fail (-22, "instance " + std::to_string (inst[k]) + " listed twice");
			seen[inst[k]] = 1;
		}
	}
	return 0;
}

bool fifoPending (const tbf_engine* e) { return e->fifoN > 0 && e->boffset < e->fifoLen; }

} // namespace

extern "C" {

int tbf_instances_clone (tbf_engine* e, uint32_t n, const uint32_t* src, uint32_t* first)
{
	if (int rc = checkInstances (e, n, src, false))
		return rc;
	const uint32_t old = (uint32_t)e->inst.size ();
	if (first)
		*first = old;
	if (n == 0)
		return 0;
	if ((uint64_t)old + n > 0x7fffffffu)
		return fail (-22, "too many instances");
	const bool dev = e->cfg.device >= 0;
	if (dev) {
		/* every launch so far done, and every source on the device (one added since the last
		 * render has only its s0: the normal new-instance upload, which the copy then carries) */
		if (int rc = engineDrain (e))
			return rc;
		if (int rc = engineDevice (e))
			return rc;
	}
	/* capture the engine-side records first: the arrays they come from grow below */
	std::vector<SlotRec> recs (n);
	try {
		for (uint32_t k = 0; k < n; k++)
			captureSlot (e, src[k], recs[k], false);
		e->inst.reserve ((size_t)old + n);
		for (uint32_t k = 0; k < n; k++) {
			Instance c = e->inst[src[k]]; /* the whole host control state, pending parts included */
			e->inst.push_back (std::move (c));
		}
	} catch (const std::bad_alloc&) {
		e->inst.resize (old);
		return fail (-12, "out of memory (instances)");
	}
	if (dev) {
		/* the arrays regrown for old + n instances (the existing ones' state moves along), then
		 * the sources' device state into the new slots */
		e->deviceReady = false;
		int rc         = engineDevice (e);
		std::vector<uint32_t> dst (n);
		for (uint32_t k = 0; k < n; k++)
			dst[k] = old + k;
		if (!rc)
			rc = moveState (e, 0, src, dst.data (), n, nullptr);
		if (!rc && hipStreamSynchronize (e->stream) != hipSuccess)
			rc = fail (-5, "k_state_move failed");
		if (rc) {
			/* nothing added: the instances go, the arrays shrink back at the next use */
			const std::string why = tbf_last_error ();
			e->inst.resize (old);
			e->retuned.erase (std::remove_if (e->retuned.begin (), e->retuned.end (), [&] (uint32_t i) { return i >= old; }),
			                  e->retuned.end ());
			e->deviceReady = false;
			if (e->devInst > old) {
				e->devInst = old;
				e->hCtl.resize (old);
				e->hProg.resize (PERSIST (old));
				e->pslot.resize (old);
			}
			return fail (rc, why);
		}
	} else
		hostPool (e, recs);
	for (uint32_t k = 0; k < n; k++) {
		installSlot (e, old + k, recs[k]);
		if ((recs[k].has & 1u) && PERSIST ((size_t)old + k + 1) <= e->hProg.size ())
			std::copy_n (e->hProg.begin () + (long)PERSIST (src[k]), PERSIST (1), e->hProg.begin () + (long)PERSIST (old + k));
	}
	if (e->fifoN > 0) {
		/* the sources' rows of the tbf_synth_sound FIFO: a clone made between two partial
		 * periods serves the same remaining frames (an instance the FIFO has not seen yet has
		 * zeros up to the next block, as tbf_synth_sound gives it) */
		const size_t       len = e->fifoLen, nn = (size_t)old + n;
		std::vector<float> L (nn * len, 0.f), R (nn * len, 0.f);
		auto row = [&] (size_t from, size_t to) {
			if (from < e->fifoN) {
				std::copy_n (e->fifoL.begin () + (long)(from * len), len, L.begin () + (long)(to * len));
				std::copy_n (e->fifoR.begin () + (long)(from * len), len, R.begin () + (long)(to * len));
			}
		};
		for (size_t i = 0; i < old; i++)
			row (i, i);
		for (uint32_t k = 0; k < n; k++)
			row (src[k], (size_t)old + k);
		e->fifoL.swap (L);
		e->fifoR.swap (R);
		e->fifoN = (uint32_t)nn;
	}
	afterInstall (e);
	return 0;
}

int tbf_instances_save (tbf_engine* e, uint32_t n, const uint32_t* inst, void* blob, uint64_t cap, uint64_t* size)
{
	if (int rc = checkInstances (e, n, inst, false))
		return rc;
	if (!size && !blob)
		return fail (-22, "null argument");
	if (fifoPending (e))
		return fail (-16, "tbf_synth_sound holds unserved frames: save and load work at block boundaries");
	if (e->cfg.device >= 0) {
		/* every launch so far done and every instance on the device, before the size query too:
		 * an instance added since the last render gets its pool entries here, which the record
		 * carries */
		if (int rc = engineDrain (e))
			return rc;
		if (int rc = engineDevice (e))
			return rc;
	}
	BlobHdr h;
	fillHeader (e, n, h);
	/* the host records' lengths */
	std::vector<BlobInst> dir (n);
	std::vector<SlotRec>  recs (n);
	uint64_t              at = h.hostOff;
	for (uint32_t k = 0; k < n; k++) {
		Writer w;
		w.at = at;
		captureSlot (e, inst[k], recs[k]);
		ioInstance (w, e->inst[inst[k]]);
		ioSlot (w, recs[k]);
		w.align (8);
		dir[k].tpl     = e->inst[inst[k]].tpl;
		dir[k].pad     = 0;
		dir[k].tplFp   = templateFingerprint (e, dir[k].tpl);
		dir[k].hostOff = at;
		dir[k].hostLen = w.at - at;
		at             = w.at;
	}
	h.devOff = align16 (at);
	h.total  = h.devOff + (uint64_t)n * h.devStride;
	if (size)
		*size = h.total;
	if (!blob)
		return 0;
	if (cap < h.total)
		return fail (-22, "blob capacity " + std::to_string (cap) + " below the " + std::to_string (h.total) + " bytes needed");
	unsigned char* B = (unsigned char*)blob;
	if (h.device && n) {
		/* the device records: packed by k_state_move, out in one copy */
		const uint64_t bytes = (uint64_t)n * h.devStride;
		if (e->stStage.cap < bytes && e->stStage.ensure (bytes))
			return fail (-12, "out of device memory (state staging)");
		std::vector<uint32_t> rec (n);
		for (uint32_t k = 0; k < n; k++)
			rec[k] = k;
		if (int rc = moveState (e, 1, inst, rec.data (), n, e->stStage.p))
			return rc;
		HIPCHK (hipMemcpyAsync (B + h.devOff, e->stStage.p, bytes, hipMemcpyDeviceToHost, e->stream));
		HIPCHK (hipStreamSynchronize (e->stream));
	}
	if (n)
		memcpy (B + sizeof (h), dir.data (), (size_t)n * sizeof (BlobInst));
	Writer w;
	w.p   = B;
	w.cap = h.devOff;
	w.at  = h.hostOff;
	for (uint32_t k = 0; k < n; k++) {
		ioInstance (w, e->inst[inst[k]]);
		ioSlot (w, recs[k]);
		w.align (8);
	}
	w.align (16);
	if (!w.ok || w.at != h.devOff)
		return fail (-5, "internal: the host records changed length while they were written");
	h.bodyHash = bodyHash (B + sizeof (h), h.total - sizeof (h));
	memcpy (B, &h, sizeof (h));
	return 0;
}

int tbf_instances_load (tbf_engine* e, uint32_t n, const uint32_t* inst, const void* blob, uint64_t size)
{
	if (int rc = checkInstances (e, n, inst, true))
		return rc;
	if (!blob)
		return fail (-22, "null argument");
	if (fifoPending (e))
		return fail (-16, "tbf_synth_sound holds unserved frames: save and load work at block boundaries");
	const unsigned char* B = (const unsigned char*)blob;
	/* everything is validated before anything is touched */
	BlobHdr b, h;
	if (size < sizeof (b))
		return fail (-22, "blob shorter than its header");
	memcpy (&b, B, sizeof (b));
	fillHeader (e, n, h);
	if (const char* f = headerMismatch (b, h))
		return fail (-22, std::string ("blob does not match this engine: ") + f);
	if (size < h.hostOff)
		return fail (-22, "blob shorter than its directory");
	/* a blob that was cut or altered anywhere: refused here, before a record is read (the
	 * records' own lengths are checked against the size all the same).  The device records
	 * hold ring positions and wheel phases that the kernels index with */
	if (b.total != size)
		return fail (-22, "blob size " + std::to_string (size) + " differs from the " + std::to_string (b.total) +
		                      " bytes its header states (truncated?)");
	if (b.bodyHash != bodyHash (B + sizeof (b), size - sizeof (b)))
		return fail (-22, "blob checksum mismatch (corrupted?)");
	std::vector<BlobInst> dir (n);
	if (n)
		memcpy (dir.data (), B + sizeof (b), (size_t)n * sizeof (BlobInst));
	std::vector<Instance> ins (n);
	std::vector<SlotRec>  recs (n);
	uint64_t              at = h.hostOff;
	for (uint32_t k = 0; k < n; k++) {
		const BlobInst& d = dir[k];
		const std::string who = "record " + std::to_string (k);
		if (d.pad)
			return fail (-22, who + ": directory entry corrupt");
		if (d.tpl >= e->tpls.size ())
			return fail (-22, who + ": template " + std::to_string (d.tpl) + " does not exist in this engine");
		if (d.tplFp != templateFingerprint (e, d.tpl))
			return fail (-22, who + ": template " + std::to_string (d.tpl) + " differs from the one the blob was saved with");
		if (d.hostOff != at || d.hostLen % 8 || d.hostLen > size - std::min (at, size))
			return fail (-22, who + ": host record outside the blob");
		Reader r;
		r.p    = B;
		r.size = at + d.hostLen;
		r.at   = at;
		ioInstance (r, ins[k]);
		ioSlot (r, recs[k]);
		r.align (8);
		if (!r.ok || r.at != at + d.hostLen)
			return fail (-22, who + ": host record truncated or corrupt");
		if (ins[k].tpl != d.tpl || ins[k].k.tpl != d.tpl)
			return fail (-22, who + ": template id differs between directory and record");
		if (ins[k].k.slabLen != e->slabLen)
			return fail (-22, who + ": reverb geometry differs");
		if ((recs[k].has & 1u) && (recs[k].prog.size () != PSLOTS * SLOT || recs[k].pslot >= PSLOTS))
			return fail (-22, who + ": program slots corrupt");
		at += d.hostLen;
	}
	if (b.devOff != align16 (at))
		return fail (-22, "blob does not match this engine: device record offset");
	if (b.total != b.devOff + (uint64_t)n * h.devStride)
		return fail (-22, "blob does not match this engine: total size");
	if (n == 0)
		return 0;
	if (h.device) {
		if (int rc = engineDrain (e))
			return rc;
		if (int rc = engineDevice (e))
			return rc;
		const uint64_t bytes = (uint64_t)n * h.devStride;
		if (e->stStage.cap < bytes && e->stStage.ensure (bytes))
			return fail (-12, "out of device memory (state staging)");
		/* in with one copy, unpacked by k_state_move; the constants from Instance::k */
		HIPCHK (hipMemcpyAsync (e->stStage.p, B + b.devOff, bytes, hipMemcpyHostToDevice, e->stream));
		std::vector<uint32_t> rec (n);
		for (uint32_t k = 0; k < n; k++)
			rec[k] = k;
		if (int rc = moveState (e, 2, rec.data (), inst, n, e->stStage.p))
			return rc;
		for (uint32_t k = 0; k < n; k++)
			HIPCHK (hipMemcpyAsync (e->cst.p + inst[k], &ins[k].k, sizeof (tbf_inst_const), hipMemcpyHostToDevice, e->stream));
		HIPCHK (hipStreamSynchronize (e->stream));
	} else
		hostPool (e, recs);
	for (uint32_t k = 0; k < n; k++) {
		ins[k].tg.tpl = e->tpls[ins[k].tpl].get ();
		e->inst[inst[k]] = std::move (ins[k]);
		installSlot (e, inst[k], recs[k]);
	}
	afterInstall (e);
	return 0;
}

/* Removal is an order-preserving compaction: survivor keep[j] (old index) becomes instance j.
 * On the device the survivors move into fresh arrays sized for the new count, in one
 * k_state_move pass (source and destination are different allocations, so no pair reads a
 * slot another pair writes, which compacting in place could not promise); the new arrays
 * replace the old ones only after the move has finished, so a failure leaves the engine as
 * it was.  Transient peak memory: the old state plus the new state (about 343 KB per
 * survivor; 1.4 GB extra when a few of 4096 instances go).  The host arrays are compacted
 * in place, ascending (j <= keep[j]: a slot is read before it is overwritten), and the
 * position-dependent fields rebased as captureSlot / installSlot do. */
int tbf_instances_remove (tbf_engine* e, uint32_t n, const uint32_t* inst, uint32_t* new_index)
{
	if (int rc = checkInstances (e, n, inst, true))
		return rc;
	const uint32_t        old = (uint32_t)e->inst.size ();
	const uint32_t        m   = old - n;
	std::vector<uint32_t> map, keep;
	try {
		map.assign (old, 0);
		for (uint32_t k = 0; k < n; k++)
			map[inst[k]] = UINT32_MAX;
		keep.reserve (m);
		for (uint32_t i = 0; i < old; i++)
			if (map[i] != UINT32_MAX) {
				map[i] = (uint32_t)keep.size ();
				keep.push_back (i);
			}
	} catch (const std::bad_alloc&) {
		return fail (-12, "out of memory (index map)");
	}
	if (n == 0) {
		if (new_index)
			std::copy (map.begin (), map.end (), new_index);
		return 0;
	}
	const bool dev = e->cfg.device >= 0;
	/* the FIFO rows of the survivors (one the FIFO has not seen yet: zeros, as a clone's) */
	std::vector<float> fL, fR;
	if (e->fifoN > 0 && m > 0) {
		try {
			const size_t len = e->fifoLen;
			fL.assign ((size_t)m * len, 0.f);
			fR.assign ((size_t)m * len, 0.f);
			for (uint32_t j = 0; j < m && keep[j] < e->fifoN; j++) {
				std::copy_n (e->fifoL.begin () + (long)(keep[j] * len), len, fL.begin () + (long)(j * len));
				std::copy_n (e->fifoR.begin () + (long)(keep[j] * len), len, fR.begin () + (long)(j * len));
			}
		} catch (const std::bad_alloc&) {
			return fail (-12, "out of memory (FIFO rows)");
		}
	}
	if (dev) {
		/* every launch so far done, and every instance on the device (one added since the last
		 * render then has its s0 there, which the move carries) */
		if (int rc = engineDrain (e))
			return rc;
		if (int rc = engineDevice (e))
			return rc;
		DevBuf<tbf_inst_state> nst;
		DevBuf<float>          nwr;
		DevBuf<double>         nsl;
		DevBuf<tbf_tgc_state>  ntg;
		DevBuf<tbf_prog_entry> npr;
		DevBuf<tbf_inst_const> ncs;
		DevBuf<tbf_seg_ctl>    nct;
		DevBuf<uint32_t>       nix;
		DevBuf<float>          ncb, nrs;
		if (m) {
			/* the sizes ensureDevice gives an engine that gets m instances at once */
			const size_t pool = PROG_POOL (m, e->devCtl);
			if (nst.ensure (m) || nwr.ensure ((size_t)m * 4 * e->wringLen) || nsl.ensure ((size_t)m * e->slabLen) ||
			    (e->devCtl && ntg.ensure (m)) || npr.ensure (pool + pool / 4) || ncs.ensure (m) ||
			    nct.ensure (2 * CTL_REGION (m)) || nix.ensure (2 * (size_t)m * TBF_CHUNK) ||
			    (e->cab.K && ncb.ensure ((size_t)m * e->cab.instFloats ())) ||
			    (e->rs.L && nrs.ensure ((size_t)m * e->rs.instFloats ()))) {
				(void)hipGetLastError ();
				return fail (-12, "out of device memory (compacted instances)");
			}
			DevSeg   into[TBF_MOVE_SEGS];
			uint32_t g = 0;
			into[g++]  = {(unsigned char*)nst.p, sizeof (tbf_inst_state)};
			into[g++]  = {(unsigned char*)nwr.p, (uint64_t)4 * e->wringLen * sizeof (float)};
			into[g++]  = {(unsigned char*)nsl.p, (uint64_t)e->slabLen * sizeof (double)};
			if (e->devCtl)
				into[g++] = {(unsigned char*)ntg.p, sizeof (tbf_tgc_state)};
			into[g++] = {(unsigned char*)npr.p, PSLOTS * SLOT * sizeof (tbf_prog_entry)};
			if (e->cab.K)
				into[g++] = {(unsigned char*)ncb.p, e->cab.instFloats () * sizeof (float)};
			if (e->rs.L)
				into[g++] = {(unsigned char*)nrs.p, e->rs.instFloats () * sizeof (float)};
			std::vector<uint32_t>       dst (m);
			std::vector<tbf_inst_const> k (m);
			for (uint32_t j = 0; j < m; j++) {
				dst[j] = j;
				k[j]   = e->inst[keep[j]].k;
			}
			if (int rc = moveState (e, 0, keep.data (), dst.data (), m, nullptr, into))
				return rc;
			HIPCHK (hipMemcpyAsync (ncs.p, k.data (), (size_t)m * sizeof (tbf_inst_const), hipMemcpyHostToDevice, e->stream));
			if (hipStreamSynchronize (e->stream) != hipSuccess)
				return fail (-5, "k_state_move failed");
		}
		/* only now: the new arrays in, the old ones (and the stage buffers, which the next render
		 * allocates for the new count) released */
		e->st    = std::move (nst);
		e->wring = std::move (nwr);
		e->rslab = std::move (nsl);
		e->tgc   = std::move (ntg);
		e->prog  = std::move (npr);
		e->cst   = std::move (ncs);
		e->ctl   = std::move (nct);
		e->ctlIdx = std::move (nix);
		e->cab.st = std::move (ncb);
		e->rs.st  = std::move (nrs);
		e->cab.wetDev.clear (); /* the mix per instance goes up again at the next cabinet call */
		e->mid0.release (), e->mid1.release (), e->mid2.release (), e->rvA.release (), e->rvB.release ();
		e->stageBlocks = e->stageN = 0;
		e->devInst     = m;
	}
	/* the host side, slot by slot; each array as far as it reaches (a host-only engine sizes
	 * its pool on demand, lastEmit / lastProg exist under device control only) */
	auto reach = [&] (size_t have) { return (size_t)(std::lower_bound (keep.begin (), keep.end (), (uint32_t)std::min<size_t> (have, old)) - keep.begin ()); };
	const size_t nCtl = e->hCtl.size (), nProg = e->hProg.size () / PERSIST (1), nSlot = e->pslot.size (),
	             nEmit = e->lastEmit.size (), nLast = e->lastProg.size ();
	for (uint32_t j = 0; j < m; j++) {
		const uint32_t i = keep[j];
		if (i == j)
			continue;
		const uint32_t shift = progBase (j) - progBase (i); /* modulo 2^32, as the offsets are */
		e->inst[j]           = std::move (e->inst[i]);
		if (i < nCtl) {
			e->hCtl[j] = e->hCtl[i];
			e->hCtl[j].prog_off += shift;
		}
		if (i < nProg)
			std::copy_n (e->hProg.begin () + (long)PERSIST (i), PERSIST (1), e->hProg.begin () + (long)PERSIST (j));
		if (i < nSlot)
			e->pslot[j] = e->pslot[i];
		if (i < nEmit) {
			e->lastEmit[j] = e->lastEmit[i];
			e->lastEmit[j].prog_off += shift;
		}
		if (i < nLast)
			e->lastProg[j] = e->lastProg[i] + shift;
	}
	e->inst.erase (e->inst.begin () + m, e->inst.end ());
	e->hCtl.resize (reach (nCtl));
	e->hProg.resize (PERSIST (reach (nProg)));
	e->pslot.resize (reach (nSlot));
	e->lastEmit.resize (reach (nEmit));
	e->lastProg.resize (reach (nLast));
	/* pending retunes: the removed instances' go, the others follow their instances */
	size_t r = 0;
	for (uint32_t i : e->retuned)
		if (map[i] != UINT32_MAX)
			e->retuned[r++] = map[i];
	e->retuned.resize (r);
	if (e->fifoN > 0) {
		e->fifoL.swap (fL);
		e->fifoR.swap (fR);
		e->fifoN = m;
	}
	/* per-chunk scratch and lists indexed by instance: the next chunk fills them again (every
	 * instance is stepped then: inAct all set, so markActive adds nothing before the rebuild) */
	e->actList.clear ();
	e->inAct.assign (m, 1);
	e->hIdent.resize (std::min<size_t> (e->hIdent.size (), m)); /* 0 .. m - 1, as dident still holds */
	e->fclean.resize (std::min<size_t> (e->fclean.size (), m));
	e->stepped.clear (), e->dhas.clear (), e->dseen.clear (), e->chg.clear (), e->curIdx.clear ();
	afterInstall (e);
	if (new_index)
		std::copy (map.begin (), map.end (), new_index);
	return 0;
}

int tbf_debug_device_bytes (const tbf_engine* e, uint64_t* instance_bytes, uint64_t* stage_bytes)
{
	if (!e)
		return fail (-22, "null argument");
	uint64_t ib = 0, sb = 0;
	if (e->cfg.device >= 0) {
		ib = e->st.cap * sizeof (tbf_inst_state) + e->wring.cap * sizeof (float) + e->rslab.cap * sizeof (double) +
		     e->tgc.cap * sizeof (tbf_tgc_state) + e->cst.cap * sizeof (tbf_inst_const) + e->ctl.cap * sizeof (tbf_seg_ctl) +
		     e->ctlIdx.cap * sizeof (uint32_t) + e->cab.st.cap * sizeof (float) +
		     e->rs.st.cap * sizeof (float);
		if (e->prog.p) /* the persistent slots of the pool (its delta part grows with a call's deltas) */
			ib += std::min<uint64_t> (PERSIST (e->devInst), e->prog.cap) * sizeof (tbf_prog_entry);
		sb = (e->mid0.cap + e->mid1.cap + e->mid2.cap) * sizeof (float) + (e->rvA.cap + e->rvB.cap) * sizeof (double);
	}
	if (instance_bytes)
		*instance_bytes = ib;
	if (stage_bytes)
		*stage_bytes = sb;
	return 0;
}

} /* extern "C" */
