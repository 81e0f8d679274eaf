/*
 * tbf_engine.cpp -- the C-ABI of include/tbf.h: instance construction (LV2 allocSynth /
 * initSynth protocol with shared tonegen templates), the host control plane, and the
 * segmentation of a render into kernel launches at block boundaries where control
 * changes.
 */
#include <hip/hip_runtime.h>
#include <assert.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <stddef.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <memory>
#include <string>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_engine_impl.h"
#include "tbf_rand.h"
#include "tbf_tpl.h"
#include "tbf_exact.h"
#include "tbf_host.h"
#include "tbf_types.h"

extern "C" int tbf_launch_stage (const tbf_launch* P, int k, hipStream_t stream);
extern "C" int tbf_chain_stages (uint32_t chain);
extern "C" uint32_t tbf_chain_kernels (uint32_t chain);

/* whether the chain runs the reverb stages (and so holds their stage buffers) */
static bool chainReverb (uint32_t chain) { return tbf_chain_stages (chain) > 2; }
/* the chain ends in the whirl (TBF_CHAIN_FULL, TBF_CHAIN_FX) */
static bool chainWhirl (uint32_t chain) { return tbf_chain_stages (chain) == TBF_NSTAGES; }
extern "C" int tbf_launch_tgctl (const tbf_launch* P, hipStream_t stream);
extern "C" int tbf_launch_front (const tbf_launch* P, hipStream_t stream);
extern "C" int tbf_launch_calibrate (int op, void* buf, uint64_t n, hipStream_t s);
extern "C" int tbf_rv_lds_fits (const tbf_inst_const* k);

using namespace tbf;

static thread_local std::string g_err;
thread_local std::vector<uint32_t>* tbf::tlAct = nullptr;

int tbf::fail (int code, const std::string& msg)
{
	g_err = msg;
	return code;
}

/* (program slots, chunk sizes and the control pool region -- SLOT, PSLOTS, PERSIST, TBF_CHUNK,
 * DPROG_CAP, CTL_REGION: tbf_engine_impl.h) */

/* ------------------------------------------------------------------ construction */

static void reverbConsts (tbf_inst_const& k, double sr, float A, float B, float C, float D, float E, float F)
{
	/* src/reverb.cpp:283-336 */
	double bq0  = ((A * 9000.0) + 1000.0) / sr;
	double b1[3] = {1.618033988749894848204586, 0.618033988749894848204586, 0.5};
	for (int q = 0; q < 3; q++) {
		double K    = tan (M_PI * bq0);
		double norm = 1.0 / (1.0 + K / b1[q] + K * K);
		k.bq[q][0]  = K * K * norm;
		k.bq[q][1]  = 2.0 * k.bq[q][0];
		k.bq[q][2]  = k.bq[q][0];
		k.bq[q][3]  = 2.0 * (K * K - 1.0) * norm;
		k.bq[q][4]  = (1.0 - K / b1[q] + K * K) * norm;
	}
	double vibSpeed    = 0.06 + C;
	double vibDepth    = (0.027 + pow (D, 3)) * 100.0;
	double size        = (pow (E, 2) * 90.0) + 10.0;
	double depthFactor = 1.0 - pow ((1.0 - (0.82 - ((B * 0.5) + (size * 0.002)))), 4);
	double blend       = 0.955 - (size * 0.007);
	double crossmod    = (F - 0.5) * 2.0;
	crossmod           = pow (crossmod, 3) * 0.5;
	double regen       = depthFactor * (0.5 - (fabs (crossmod) * 0.031));
	static const double depth[8] = {0.003251, 0.002999, 0.002917, 0.002749, 0.002503, 0.002423, 0.002146, 0.002088};
	static const int    dmul[12] = {79, 73, 71, 67, 61, 59, 53, 47, 43, 41, 37, 31};
	for (int l = 0; l < 8; l++)
		k.vibDelta[l] = depth[l] * vibSpeed;
	k.vibDepth      = vibDepth;
	k.blend         = blend;
	k.crossmod      = crossmod;
	k.oneMinusAbsCm = 1.0 - fabs (crossmod);
	k.regen         = regen;
	for (int l = 0; l < 12; l++)
		k.delay[l] = (int)(dmul[l] * size);
	k.delay[12] = (int)((29 * size) - (56 * size * fabs (crossmod)));
	uint32_t o  = 0;
	for (int c = 0; c < 2; c++)
		for (int l = 0; l < 13; l++) {
			k.ringOff[c * 13 + l] = o;
			/* line 12 of channel 0 holds the predelay history (TBF_PD_HIST floats) instead
			 * of a ring; channel 1's stays unused */
			const int len = (l == 12 && c == 0) ? std::max (k.delay[l] + 1, TBF_PD_HIST / 2) : k.delay[l] + 1;
			o += (uint32_t)((len + TBF_RING_ALIGN - 1) & ~(TBF_RING_ALIGN - 1));
		}
	k.slabLen = o;
}

static void whirlConsts (tbf_inst_const& k, const WhirlTables& wt, const Config& c)
{
	memcpy (k.drf, wt.drf, sizeof (k.drf));
	memcpy (k.hornSpacing, wt.hornSpacing, sizeof (k.hornSpacing));
	memcpy (k.drumSpacing, wt.drumSpacing, sizeof (k.drumSpacing));
	memcpy (k.hornPhase, wt.phase, sizeof (k.hornPhase));
	/* initialize (src/whirl.cpp:626-662): leakage = leakLevel * hornLevel */
	k.leakage   = c.leakLevel * c.hornLevel;
	k.hornLevel = c.hornLevel;
	/* mic widths (fsetHornMicWidth / fsetDrumMicWidth, src/whirl.cpp:912-949; width 0
	 * leaves the initValues gains hll dll hrr drr = 1, others 0) */
	float hll = 1.f, hlr = 0.f, hrl = 0.f, hrr = 1.f, dll = 1.f, dlr = 0.f, drl = 0.f, drr = 1.f;
	if (c.drumMicWidth != 0.f) {
		const float dw = c.drumMicWidth;
		const float dwP = dw > 0.f ? (dw > 1.f ? 1.f : dw) : 0.f;
		const float dwN = dw < 0.f ? (dw < -1.f ? 1.f : -dw) : 0.f;
		dll = sqrtf (1.f - dwP);
		dlr = sqrtf (0.f + dwP);
		drl = sqrtf (0.f + dwN);
		drr = sqrtf (1.f - dwN);
	}
	if (c.hornMicWidth != 0.f) {
		const float hw = c.hornMicWidth;
		const float hwP = hw > 0.f ? (hw > 1.f ? 1.f : hw) : 0.f;
		const float hwN = hw < 0.f ? (hw < -1.f ? 1.f : -hw) : 0.f;
		hll = sqrtf (1.f - hwP);
		hlr = sqrtf (0.f + hwP);
		hrl = sqrtf (0.f + hwN);
		hrr = sqrtf (1.f - hwN);
	}
	const float mic[8] = {hll, hlr, dll, dlr, hrl, hrr, drl, drr};
	memcpy (k.mic, mic, sizeof (mic));
	/* HN_MOTION / DR_MOTION angle offsets (src/whirl.cpp:1396-1400) */
	k.fwAng = c.micAngle * .25;
	k.bwAng = 1. + c.micAngle * -.25;
	k.deadzone = (.05 / (60.f * wt.sr));
	memcpy (k.revHorn, wt.revHorn, sizeof (k.revHorn));
	memcpy (k.revDrum, wt.revDrum, sizeof (k.revDrum));
	k.hnHardstop = (float)(10.f / (60.f * wt.sr));
	k.drHardstop = (float)(8.f / (60.f * wt.sr));
	k.minspeed   = (float)(3.f / (60.f * wt.sr));
	k.hnLimit    = (float)(60.f / (60. * wt.sr));
	k.drLimit    = (float)(100.f / (60. * wt.sr));
	k.sr         = wt.sr;
}

/* fsetCharacter (src/overdrive.cpp:547-574): character A and the linear-segment output
 * level C */
void tbf::setCharacter (Instance& in, float value)
{
	static const double Aval[5] = {0.0, 0.25, 0.50, 0.75, 1.00};
	static const double Cval[5] = {1.0, 0.70, 0.25, 0.15, 0.13};
	in.odA                      = value;
	for (int q = 0; q < 4; q++)
		if (value <= Aval[q + 1]) {
			float a = (float)Aval[q], b = (float)Aval[q + 1], p = (float)Cval[q], qq = (float)Cval[q + 1];
			in.odC  = p + (value - a) * (qq - p) / (b - a);
			break;
		}
	in.ctlDirty = true;
}

/* the engine-wide tables the cfg shapes: whirl displacement / IR tables, filters and
 * speeds (initWhirl, src/whirl.cpp:956-986), the compact ring window derived from the
 * geometry, the scanner's offset tables and stator increment (init_vibrato,
 * src/vibrato.cpp:312-317) */
static int buildShared (tbf_engine* e)
{
	const double sr = e->cfg.sample_rate;
	e->wt.build (sr, e->conf);
	e->engFp = 0;
	/* compact whirl ring: live window < maxAhead + 2 + one sub-block */
	uint32_t W = 512;
	while ((float)W < e->wt.maxAhead + 2.0f + TBF_SUB + 2.0f)
		W *= 2;
	if (W > 2048)
		return fail (-22, "whirl write-ahead exceeds the reference ring (2048 samples): geometry out of range");
	/* The smallest write-ahead the whirl kernels render exactly.  The reference adds sample
	 * m's motions at slots floor (t), floor (t) + 1 with t = spacing + intp + (float)outpos
	 * and only then reads and clears slot outpos (src/whirl.cpp:1432-1469, 1590-1612), so
	 * an add with a lead under the distance to a later sample of the block is heard by
	 * that sample.
	 *   k_whirl: the 64 lanes of a sub-block starting at outpos B read and clear slots
	 *   B .. B + 63 of all four rings before any of the sub-block's adds (the fast passes
	 *   and the serial replay alike).  Sample m's add at slot s in [B + m, B + 63] is read
	 *   by sample s - B of this sub-block in the reference, but one ring length late here;
	 *   any s >= B + 64 is read by a later sub-block, after the add, as in the reference.
	 *   Exact iff floor (t) >= B + 64 for every m >= 0, i.e. for m = 0: lead >= TBF_SUB.
	 *   k_whirl_split: the horn wave reads and clears its window like k_whirl.  The drum
	 *   wave leaves dL / dR in window k, the horn wave reads them behind the barrier the
	 *   drum wave passes before its adds of sub-block k, and window k is cleared behind
	 *   the next barrier.  An add of sub-block k inside window k would race with that
	 *   read and then be cleared; from B + 64 on it lands in windows not yet consumed.
	 *   The same condition: lead >= TBF_SUB.
	 * Rounding: minAhead = fl (spacing + min table value).  intp = fl (fl (x fl (1 - hd)) +
	 * fl (hd y)) with fl (1 - hd) + hd >= 1 - 2^-25 and three roundings of 2^-24 each is
	 * >= min (x, y) (1 - 3.5 * 2^-24), at most 2048 * 3.5 * 2^-24 = 4.3e-4 under the table's
	 * minimum (a table value is below the 2048-sample ring), and fl (spacing + intp), an
	 * ulp of 7.6e-6 at 64, is monotone in intp: with minAhead >= 64 + 2^-10 it is >= 64.
	 * Then spacing + intp + outpos >= 64 + outpos, an integer a float holds exactly up to
	 * outpos 2047, so the last rounding cannot go below it and floor (t) >= outpos + 64.
	 * Chains that end before the whirl (tonegen, preamp and reverb taps) have no bound. */
	if (tbf_chain_stages (e->cfg.chain_mode) == TBF_NSTAGES && !(e->wt.minAhead >= TBF_WH_MIN_LEAD)) {
		char msg[200];
		snprintf (msg, sizeof msg,
		          "whirl write-ahead %.3f samples is under the %.3f the whirl kernels render exactly: sample rate too low "
		          "or microphone too near the rotors",
		          (double)e->wt.minAhead, (double)TBF_WH_MIN_LEAD);
		return fail (-22, msg);
	}
	e->wringLen = W;
	/* vibrato tables (src/vibrato.cpp:91-95, 224-251) */
	e->vibTab.resize (3 * 2048);
	const double amp[3] = {e->conf.vib1OffAmp, e->conf.vib2OffAmp, e->conf.vib3OffAmp};
	for (int t = 0; t < 3; t++)
		for (int i = 0; i < 2048; i++) {
			double m                = sin ((2.0 * M_PI * i) / 2048);
			e->vibTab[t * 2048 + i] = (unsigned int)((1.0 + amp[t] + (m * amp[t])) * 65536.0);
		}
	e->statorInc = (unsigned int)(((e->conf.vibFqHertz * 2048) / sr) * 65536.0);
	return 0;
}

/* host worker threads for per-template work: the process's lease (OMP_NUM_THREADS, set
 * on the GPU boxes) or the hardware, at most TBF_MAX_HOST_THREADS */
unsigned tbf::hostThreads ()
{
	unsigned    t   = std::thread::hardware_concurrency ();
	const char* omp = getenv ("OMP_NUM_THREADS");
	const char* ht  = getenv ("TBF_HOST_THREADS");
	if (ht && atoi (ht) > 0)
		t = (unsigned)atoi (ht);
	else if (omp && atoi (omp) > 0)
		t = (unsigned)atoi (omp);
	return std::max (1u, std::min (t, TBF_MAX_HOST_THREADS));
}

/* A persistent pool of hostThreads () - 1 workers (the caller is the last): a dense-event
 * chunk runs several parallel sections, and creating 16 threads for each cost ~0.3-0.8 ms.
 * One job at a time (the mutex), so engines driven from several host threads share it.
 * A job ends when its tasks are done, not when every worker has woken: each job is its own
 * object, so a worker the OS schedules late finds that job's tasks taken and leaves it. */
class HostPool {
  public:
	static HostPool& get ()
	{
		static HostPool p;
		return p;
	}
	void run (uint32_t n, const std::function<void (uint32_t)>& f)
	{
		std::lock_guard<std::mutex> job (jobM);
		auto                        j = std::make_shared<Job> ();
		j->fn                         = &f;
		j->cnt                        = n;
		{
			std::lock_guard<std::mutex> g (m);
			cur = j;
			gen++;
		}
		cv.notify_all ();
		work (*j);
		std::unique_lock<std::mutex> g (m);
		done.wait (g, [&] { return j->finished.load () == n; });
		cur.reset ();
	}
	unsigned workers () const { return (unsigned)th.size () + 1; }

  private:
	struct Job {
		const std::function<void (uint32_t)>* fn  = nullptr;
		uint32_t                              cnt = 0;
		std::atomic<uint32_t>                 next {0}, finished {0};
	};
	HostPool ()
	{
		const unsigned nt = hostThreads ();
		for (unsigned k = 1; k < nt; k++)
			th.emplace_back ([this] { loop (); });
	}
	~HostPool ()
	{
		{
			std::lock_guard<std::mutex> g (m);
			quit = true;
		}
		cv.notify_all ();
		for (auto& t : th)
			t.join ();
	}
	void work (Job& j)
	{
		for (uint32_t t; (t = j.next.fetch_add (1)) < j.cnt;) {
			(*j.fn) (t);
			if (j.finished.fetch_add (1) + 1 == j.cnt) {
				std::lock_guard<std::mutex> g (m);
				done.notify_all ();
			}
		}
	}
	void loop ()
	{
		uint64_t seen = 0;
		for (;;) {
			std::shared_ptr<Job> j;
			{
				std::unique_lock<std::mutex> g (m);
				cv.wait (g, [&] { return quit || gen != seen; });
				if (quit)
					return;
				seen = gen;
				j    = cur;
			}
			if (j)
				work (*j);
		}
	}
	std::vector<std::thread> th;
	std::mutex               m, jobM;
	std::condition_variable  cv, done;
	std::shared_ptr<Job>     cur;
	uint64_t                 gen  = 0;
	bool                     quit = false;
};

/* run f(t) for t < n on up to hostThreads () threads */
void tbf::parallelFor (uint32_t n, const std::function<void (uint32_t)>& f)
{
	if (n <= 1 || hostThreads () <= 1) {
		for (uint32_t t = 0; t < n; t++)
			f (t);
		return;
	}
	HostPool::get ().run (n, f);
}

extern "C" {

int tbf_abi_version (void) { return TBF_ABI_VERSION; }
const char* tbf_last_error (void) { return g_err.c_str (); }

int tbf_engine_create (const tbf_engine_config* cfg, tbf_engine** out)
{
	if (!cfg || !out)
		return fail (-22, "null argument");
	if (!(cfg->sample_rate >= 8000.0 && cfg->sample_rate <= 192000.0))
		return fail (-22, "sample_rate out of range");
	if (cfg->whirl_out != TBF_WHIRL_OUT_MIC && cfg->whirl_out != TBF_WHIRL_OUT_DIRECT)
		return fail (-22, "whirl_out: not a TBF_WHIRL_OUT_* value");
	if (cfg->whirl_out != TBF_WHIRL_OUT_MIC && !chainWhirl (cfg->chain_mode))
		return fail (-22, "whirl_out: TBF_WHIRL_OUT_DIRECT needs a chain that runs the whirl (TBF_CHAIN_FULL, TBF_CHAIN_FX)");
	/* device -1: host-only engine (table builders and control plane; render refuses) */
	if (cfg->device != -1) {
		int ndev = 0;
		if (hipGetDeviceCount (&ndev) != hipSuccess || ndev <= 0)
			return fail (-19, "no HIP device available");
		if (cfg->device < 0 || cfg->device >= ndev)
			return fail (-19, "device ordinal out of range");
	}
	std::unique_ptr<tbf_engine> e (new tbf_engine ());
	e->cfg = *cfg;
	if (cfg->device >= 0) {
		HIPCHK (hipSetDevice (cfg->device));
		/* stream creation order matters: the process has GPU_MAX_HW_QUEUES (4) hardware
		 * queues and streams take them round-robin at creation.  The engine's own stream
		 * first, then the three stage-group streams: a caller's stream created after the
		 * engine shares the engine stream's queue (idle when the caller passes its
		 * stream); one created before shares the last stage group's, whose work the
		 * caller's stream waits for anyway.  A stage group's queue shared with the
		 * caller's stream would order the group's next launches behind the caller's
		 * end-of-call wait (measured with a fifth engine stream: steady step 6.7 -> 8.1 ms) */
		HIPCHK (hipStreamCreateWithFlags (&e->stream, hipStreamNonBlocking));
		if (const char* pg = getenv ("TBF_PIPE_GROUPS")) { /* "g0,...,g5": groups 0..5, non-decreasing, from 0 */
			/* stages 0 and 1 always share a stream: the tonegen-only chain's mixFixed flags
			 * (one buffer for every chunk) are written by k_tonegen and read by k_mixpre */
			for (int k = 0; k < TBF_NSTAGES && *pg; k++) {
				const int g = atoi (pg);
				if (g >= 0 && g < TBF_NSTAGES && (k == 0 ? g == 0 : k == 1 ? g == e->grp[0] : (g >= e->grp[k - 1] && g <= e->grp[k - 1] + 1)))
					e->grp[k] = g;
				while (*pg && *pg != ',')
					pg++;
				if (*pg == ',')
					pg++;
			}
		}
		/* stage-group stream priorities (TBF_GROUP_PRIO="p0,p1,...": HIP stream priorities,
		 * lower = higher, clamped to the device's range; default: the reverb group high).
		 * The reverb group is the step's critical path (k_rv_pre -> k_rv_core_lds ->
		 * k_rv_post, ~65 ms alone per 2048 blocks against ~46 for k_tonegen + k_mixpre and ~37
		 * for k_whirl); at equal priority the other groups' workgroups took the CUs first
		 * and k_rv_pre ran 4x slower than alone (tools/timeline.py, profiles/r05/s23) */
		int pLeast = 0, pGreatest = 0;
		HIPCHK (hipDeviceGetStreamPriorityRange (&pLeast, &pGreatest));
		int prio[TBF_NSTAGES] = {0, 0, 0, 0, 0, 0};
		if (e->grp[2] == e->grp[3] && e->grp[3] == e->grp[4] && e->grp[2] != e->grp[1] && e->grp[4] != e->grp[5])
			prio[e->grp[2]] = pGreatest;
		if (const char* gp = getenv ("TBF_GROUP_PRIO"))
			for (int g = 0; g < TBF_NSTAGES && *gp; g++) {
				prio[g] = atoi (gp);
				while (*gp && *gp != ',')
					gp++;
				if (*gp == ',')
					gp++;
			}
		for (int g = 0; g <= e->grp[TBF_NSTAGES - 1]; g++) {
			const int p = std::min (std::max (prio[g], std::min (pLeast, pGreatest)), std::max (pLeast, pGreatest));
			HIPCHK (hipStreamCreateWithPriority (&e->gs[g], hipStreamNonBlocking, p));
		}
		for (int k = 0; k < TBF_NSTAGES; k++) {
			HIPCHK (hipEventCreateWithFlags (&e->sdone[k], hipEventDisableTiming));
			for (int p = 0; p < 4; p++)
				HIPCHK (hipEventCreateWithFlags (&e->pev[p][k], hipEventDisableTiming));
		}
		HIPCHK (hipEventCreateWithFlags (&e->sjoin, hipEventDisableTiming));
		/* TBF_RV_LDS=0: the streaming reverb core (k_rv_core) instead of k_rv_core_lds */
		if (const char* rl = getenv ("TBF_RV_LDS"))
			e->rvLdsOn = rl[0] != '0';
		/* k_rv_core_lds runs one persistent workgroup per CU (TBF_RV_PERSIST=0: one per
		 * instance and channel, the round-2 grid) */
		int ncu = 0;
		HIPCHK (hipDeviceGetAttribute (&ncu, hipDeviceAttributeMultiprocessorCount, cfg->device));
		if (const char* ts = getenv ("TBF_TG_SPLIT"))
			e->tgSplit = atoi (ts);
		if (const char* sc = getenv ("TBF_STEADY_CHUNK")) /* A/B: blocks per chunk without deltas */
			e->steadyChunk = (uint32_t)std::min (std::max (atoi (sc), TBF_CHUNK), TBF_STEADY_MAX);
		const char* rp = getenv ("TBF_RV_PERSIST"); /* 0: per-pair grid; n > 0: n workgroups */
		e->rvGrid      = rp ? (uint32_t)std::max (atoi (rp), 0) : (uint32_t)std::max (ncu, 1);
		if (e->rvWork.ensure (1))
			return fail (-12, "out of device memory");
		for (ChunkStaging& cs : e->stg)
			HIPCHK (hipEventCreateWithFlags (&cs.upEv, hipEventDisableTiming));
		const char* pl = getenv ("TBF_PIPELINE");
		e->pipeline    = !(pl && pl[0] == '0');
		if (const char* pa = getenv ("TBF_PRE_AHEAD")) /* 0 / 1: the next chunk's k_rv_pre beside k_rv_post (A/B) */
			e->preAhead = pa[0] == '1';
		/* TBF_HOST_CONTROL=1: the per-wheel tone-generator control on the host (the
		 * reference path for A/B); default: on the device (k_tgctl) */
		const char* hc = getenv ("TBF_HOST_CONTROL");
		e->devCtl      = !(hc && hc[0] == '1');
		const char* hs = getenv ("TBF_HOST_SERIAL"); /* the serial loop (A/B); TBF_HOST_THREADS: workers */
		e->parCtl      = !(hs && hs[0] == '1');
		e->dbgPhases   = getenv ("TBF_DEBUG_HOST_PHASES") != nullptr;
		const char* df = getenv ("TBF_DEVICE_FRONT"); /* 0: note-only chunks step on the host too (A/B) */
		e->frontOn     = !(df && df[0] == '0');
		if (const char* sp = getenv ("TBF_WHIRL_SPLIT")) /* 0 / 1: k_whirl / k_whirl_split always */
			e->whSplit = sp[0] != '0' ? 1 : 0;
		e->nCU = (uint32_t)std::max (ncu, 1);
		if (const char* fm = getenv ("TBF_FRONT_MIN")) /* events a chunk needs for the device front end */
			e->frontMin = (uint32_t)std::max (atoi (fm), 1);
	}
	if (int rc = buildShared (e.get ()))
		return rc;
	*out = e.release ();
	return 0;
}

int tbf_engine_destroy (tbf_engine* e)
{
	if (!e)
		return 0;
	if (e->cfg.device >= 0)
		(void)hipSetDevice (e->cfg.device);
	if (e->stream)
		(void)hipStreamSynchronize (e->stream);
	for (hipStream_t q : e->gs)
		if (q)
			(void)hipStreamSynchronize (q);
	if (e->stream)
		(void)hipStreamDestroy (e->stream);
	for (hipStream_t q : e->gs)
		if (q)
			(void)hipStreamDestroy (q);
	for (int k = 0; k < TBF_NSTAGES; k++) {
		if (e->sdone[k])
			(void)hipEventDestroy (e->sdone[k]);
		for (int p = 0; p < 4; p++)
			if (e->pev[p][k])
				(void)hipEventDestroy (e->pev[p][k]);
	}
	if (e->sjoin)
		(void)hipEventDestroy (e->sjoin);
	for (ChunkStaging& cs : e->stg)
		if (cs.upEv)
			(void)hipEventDestroy (cs.upEv);
	delete e; /* the device buffers go with it (DevBuf) */
	return 0;
}

int tbf_template_create (tbf_engine* e, const double* mts128, const double* ratio9, uint32_t seed, uint32_t* id)
{
	if (!e || !id)
		return fail (-22, "null argument");
	std::unique_ptr<TgTemplate> t (new TgTemplate ());
	t->build (e->cfg.sample_rate, mts128, ratio9, seed, e->conf);
	*id = (uint32_t)e->tpls.size ();
	e->tpls.push_back (std::move (t));
	e->deviceReady = false;
	return 0;
}

int tbf_templates_create (tbf_engine* e, uint32_t n, const double* mts128, const double* ratio9, const uint32_t* seeds,
                          uint32_t* ids)
{
	if (!e || (n && (!seeds || !ids)))
		return fail (-22, "null argument");
	if (!e->stream)
		return fail (-19, "device template construction needs a device engine");
	if (n == 0)
		return 0;
	HIPCHK (hipSetDevice (e->cfg.device));
	const double                             sr = e->cfg.sample_rate;
	std::vector<std::unique_ptr<TgTemplate>> ts (n);
	std::vector<uint32_t>                    E (61 * (size_t)n);
	std::vector<uint64_t>                    total (n), base (n);
	std::vector<tbf_tpl_wheel>               wh ((size_t)n * TBF_NW);
	uint64_t                                 sum = 0;
	uint32_t                                 maxChunks = 0, maxLen = 0;
	/* the play matrices on the device (k_tpl_matrix) unless TBF_HOST_MATRIX=1 (A/B: the
	 * host builder of tbf_template_create, one template per host thread) */
	const char* hm         = getenv ("TBF_HOST_MATRIX");
	const bool  hostMatrix = hm && atoi (hm) != 0;
	/* the rand-free tables of each template (frequencies, wheel lengths and spectra) and
	 * its rand() window, one template per host thread */
	parallelFor (n, [&] (uint32_t t) {
		ts[t].reset (new TgTemplate ());
		ts[t]->prepare (sr, mts128 ? mts128 + 128 * (size_t)t : nullptr, ratio9 ? ratio9 + 9 * (size_t)t : nullptr,
		                e->conf, hostMatrix);
		uint32_t  W[31];
		GlibcRand rnd (seeds[t]);
		rnd.window (W);
		gr_extend (W, &E[61 * (size_t)t]);
	});
	for (uint32_t t = 0; t < n; t++) {
		TgTemplate& T = *ts[t];
		total[t] = T.total;
		base[t]  = sum;
		sum += T.total;
		maxChunks = std::max (maxChunks, (uint32_t)((T.total + 511) / 512));
		for (int i = 1; i <= TBF_NW; i++) {
			tbf_tpl_wheel& w = wh[(size_t)t * TBF_NW + i - 1];
			memset (&w, 0, sizeof (w));
			w.off = T.off[i];
			w.len = T.len[i];
			w.np  = T.nPartials[i];
			w.U   = T.U[i];
			for (int q = 0; q < w.np; q++) {
				w.amp[q] = T.pAmp[i][q];
				w.hz[q]  = T.pHz[i][q];
			}
			maxLen = std::max (maxLen, w.len);
		}
	}
	DevBuf<uint32_t>      dE;
	DevBuf<uint64_t>      dTot, dBase;
	DevBuf<tbf_tpl_wheel> dWh;
	DevBuf<uint8_t>       dLsb;
	DevBuf<float>         dBank;
	/* play matrix: the cfg-only inputs, each template's frequencies and bus ratios */
	MatrixInputs          mi;
	const size_t          nk = (size_t)n * 384;
	std::vector<double>   fr, ra;
	DevBuf<tbf_le>        dTm, dTp, dXt;
	DevBuf<uint32_t>      dTmOff, dTpOff, dXtOff, dCnt, dOff;
	DevBuf<float>         dTaper;
	DevBuf<double>        dFr, dRa;
	DevBuf<tbf_contrib>   dStage, dOut;
	std::vector<uint32_t> hCnt, hOff;
	std::vector<Contrib>  hOut;
	if (!hostMatrix) {
		mi.build (e->conf);
		fr.resize ((size_t)n * TBF_NW);
		ra.resize ((size_t)n * 9);
		for (uint32_t t = 0; t < n; t++) {
			memcpy (&fr[(size_t)t * TBF_NW], ts[t]->frequency, TBF_NW * sizeof (double));
			memcpy (&ra[(size_t)t * 9], ts[t]->targetRatio, 9 * sizeof (double));
		}
		if (dTm.ensure (mi.tm.size ()) || dTp.ensure (mi.tp.size ()) || dXt.ensure (mi.xt.size ()) ||
		    dTmOff.ensure (mi.tmOff.size ()) || dTpOff.ensure (mi.tpOff.size ()) || dXtOff.ensure (mi.xtOff.size ()) ||
		    dTaper.ensure (128 * 9) || dFr.ensure (fr.size ()) || dRa.ensure (ra.size ()) || dCnt.ensure (nk) ||
		    dOff.ensure (nk + 1) || dStage.ensure (nk * mi.cap) || dOut.ensure (nk * mi.cap))
			return fail (-12, "device play matrix buffers");
	}
	auto releaseAll = [&] () {
		dE.release (), dTot.release (), dBase.release (), dWh.release (), dLsb.release (), dBank.release ();
		dTm.release (), dTp.release (), dXt.release (), dTmOff.release (), dTpOff.release (), dXtOff.release ();
		dTaper.release (), dFr.release (), dRa.release (), dCnt.release (), dOff.release (), dStage.release ();
		dOut.release ();
	};
	if (dE.ensure (E.size ()) || dTot.ensure (n) || dBase.ensure (n) || dWh.ensure (wh.size ()) || dLsb.ensure (sum) ||
	    dBank.ensure (sum)) {
		releaseAll ();
		return fail (-12, "device template buffers");
	}
	int rc = 0;
	std::vector<float> hb (sum);
	do {
		hipStream_t s = e->stream;
		if (hipMemcpyAsync (dE.p, E.data (), E.size () * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
		    hipMemcpyAsync (dTot.p, total.data (), n * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
		    hipMemcpyAsync (dBase.p, base.data (), n * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
		    hipMemcpyAsync (dWh.p, wh.data (), wh.size () * sizeof (tbf_tpl_wheel), hipMemcpyHostToDevice, s) != hipSuccess) {
			rc = fail (-5, "template upload");
			break;
		}
		if (tbf_tpl_launch (n, maxChunks, maxLen, dE.p, dTot.p, dBase.p, dWh.p, dLsb.p, dBank.p, sr, s)) {
			rc = fail (-5, "template kernels");
			break;
		}
		if (!hostMatrix) {
			auto up = [&] (void* d, const void* h, size_t bytes) {
				return bytes == 0 || hipMemcpyAsync (d, h, bytes, hipMemcpyHostToDevice, s) == hipSuccess;
			};
			if (!up (dTm.p, mi.tm.data (), mi.tm.size () * sizeof (tbf_le)) ||
			    !up (dTp.p, mi.tp.data (), mi.tp.size () * sizeof (tbf_le)) ||
			    !up (dXt.p, mi.xt.data (), mi.xt.size () * sizeof (tbf_le)) ||
			    !up (dTmOff.p, mi.tmOff.data (), mi.tmOff.size () * 4) ||
			    !up (dTpOff.p, mi.tpOff.data (), mi.tpOff.size () * 4) ||
			    !up (dXtOff.p, mi.xtOff.data (), mi.xtOff.size () * 4) || !up (dTaper.p, mi.taper, sizeof (mi.taper)) ||
			    !up (dFr.p, fr.data (), fr.size () * 8) || !up (dRa.p, ra.data (), ra.size () * 8)) {
				rc = fail (-5, "play matrix upload");
				break;
			}
			const tbf_tpl_mx mx = {dTm.p,    dTmOff.p,    dTp.p,       dTpOff.p,    dXt.p, dXtOff.p,
			                       dTaper.p, mi.wiringXT, mi.floor, mi.minLevel, mi.cap};
			hCnt.resize (nk);
			hOff.resize (nk + 1);
			if (tbf_tpl_matrix_launch (n, &mx, dFr.p, dRa.p, dStage.p, dCnt.p, dOff.p, dOut.p, s)) {
				rc = fail (-5, "play matrix kernels");
				break;
			}
			if (hipMemcpyAsync (hCnt.data (), dCnt.p, nk * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
			    hipMemcpyAsync (hOff.data (), dOff.p, (nk + 1) * 4, hipMemcpyDeviceToHost, s) != hipSuccess) {
				rc = fail (-5, "play matrix download");
				break;
			}
		}
		if (hipMemcpyAsync (hb.data (), dBank.p, sum * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
		    hipStreamSynchronize (s) != hipSuccess) {
			rc = fail (-5, "template download");
			break;
		}
		if (!hostMatrix) {
			for (size_t q = 0; q < nk; q++)
				if (hCnt[q] > mi.cap) {
					rc = fail (-5, "play matrix list longer than its staging");
					break;
				}
			if (rc)
				break;
			static_assert (sizeof (Contrib) == sizeof (tbf_contrib), "Contrib is tbf_contrib's layout");
			hOut.resize (hOff[nk]);
			if ((hOff[nk] && hipMemcpyAsync (hOut.data (), dOut.p, hOff[nk] * sizeof (Contrib), hipMemcpyDeviceToHost,
			                                 s) != hipSuccess) ||
			    hipStreamSynchronize (s) != hipSuccess) {
				rc = fail (-5, "play matrix download");
				break;
			}
		}
	} while (0);
	releaseAll ();
	if (rc)
		return rc;
	parallelFor (n, [&] (uint32_t t) {
		TgTemplate& T = *ts[t];
		if (!hostMatrix)
			for (int k = 0; k < 384; k++) {
				const size_t q = (size_t)t * 384 + k;
				T.keyContrib[k].assign (hOut.begin () + hOff[q], hOut.begin () + hOff[q + 1]);
			}
		T.bank.assign (hb.begin () + base[t], hb.begin () + base[t] + total[t]);
		GlibcRand rnd (seeds[t]);
		rnd.discard (T.total); /* the draws of the bank */
		T.finish (rnd);
	});
	for (uint32_t t = 0; t < n; t++) {
		ids[t] = (uint32_t)e->tpls.size ();
		e->tpls.push_back (std::move (ts[t]));
	}
	e->deviceReady = false;
	return 0;
}

int tbf_template_bank (tbf_engine* e, uint32_t tid, float* out, uint64_t cap, uint32_t* lens)
{
	if (!e || tid >= e->tpls.size ())
		return fail (-22, "bad template id");
	const TgTemplate& t = *e->tpls[tid];
	if (lens)
		for (int i = 1; i <= TBF_NW; i++)
			lens[i - 1] = t.len[i];
	if (out) {
		if (cap < t.bank.size ())
			return fail (-28, "buffer too small");
		memcpy (out, t.bank.data (), t.bank.size () * sizeof (float));
	}
	return (int)t.bank.size ();
}

/* the CLAP parameters' default values (clap_plugin_params get_info, src/clap.cpp:383-545;
 * the plugin's init copies them into its parameter array, 1062-1067) */
static void clapParamDefaults (double* params)
{
	static const float drawbar[9] = {7.0f, 8.0f, 8.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
	static const float top[9] = {1, 3, 1, 2, 3, 4, 5, 6, 8}, bottom[9] = {2, 2, 1, 1, 1, 1, 1, 1, 1};
	for (int i = 0; i < 64; i++)
		params[i] = 0.0;
	for (int i = 0; i < 9; i++) {
		params[TBF_P_DRAWBAR_MIN + i] = drawbar[i];
		params[20 + i]                = top[i];    /* P_RATIO_TOP_MIN */
		params[29 + i]                = bottom[i]; /* P_RATIO_BOTTOM_MIN */
	}
	params[TBF_P_DRUM]   = 1.0f;
	params[TBF_P_HORN]   = 1.0f;
	params[TBF_P_REVERB] = 0.1f;
}

int tbf_instances_add (tbf_engine* e, uint32_t n, const uint32_t* tpl_ids, const uint32_t* seeds, uint32_t* first)
{
	if (!e || (n && (!tpl_ids || !seeds)))
		return fail (-22, "null argument");
	const double sr = e->cfg.sample_rate;
	if (first)
		*first = (uint32_t)e->inst.size ();
	for (uint32_t q = 0; q < n; q++) {
		if (tpl_ids[q] >= e->tpls.size ())
			return fail (-22, "bad template id");
		e->everAdded = true;
		e->inst.emplace_back ();
		Instance& in = e->inst.back ();
		in.tpl       = tpl_ids[q];
		in.ctlRand   = GlibcRand (seeds[q] ^ 0x5bd1e995u);
		memset (&in.k, 0, sizeof (in.k));
		memset (&in.s0, 0, sizeof (in.s0));
		memset (&in.ctl, 0, sizeof (in.ctl));
		clapParamDefaults (in.params);
		in.k.tpl = in.tpl;
		/* allocSynth order: allocReverb (rand x16 vib phases, fpdL, fpdR), allocWhirl,
		 * allocTonegen, allocPreamp (rand fpd)  -- b_synth/lv2.cpp:336-353 */
		GlibcRand rnd (seeds[q]);
		for (int c = 0; c < 2; c++)
			for (int l = 0; l < 8; l++)
				in.s0.rv.ch[c].vib[l] = rnd.next () - 2147483647 / 2;
		uint32_t f = 1;
		while (f < 16386)
			f = (uint32_t)rnd.next () * 0xFFFFFFFFu;
		in.s0.rv.fpdL = f;
		f          = 1;
		while (f < 16386)
			f = (uint32_t)rnd.next () * 0xFFFFFFFFu;
		in.s0.rv.fpdR = f;
		in.s0.rv.fpdL2 = in.s0.rv.fpdL;
		in.s0.rv.fpdR2 = in.s0.rv.fpdR;
		f          = 1;
		while (f < 16386)
			f = (uint32_t)rnd.next () * 0xFFFFFFFFu;
		in.s0.mo.odFpd  = f;
		in.s0.mo.fpFlip = 1;
		in.s0.rv.pdAge = 0; /* countM = 1 and zeroed rings: the first delayM outputs are 0 */
		in.s0.rv.pdPos = 0;
		for (int c = 0; c < 2; c++)
			for (int l = 0; l < 12; l++)
				in.s0.rv.ch[c].count[l] = 1;
		reverbConsts (in.k, sr, 1.0f, 0.2f, 0.0f, 0.0f, 0.4f, 0.8f);
		if (in.k.delay[12] < 0 || in.k.delay[12] >= TBF_PD_HIST) /* 560 at the fixed settings */
			return fail (-22, "predelay longer than its history");
		whirlConsts (in.k, e->wt, e->conf);
		in.whr.init (e->wt.sr, e->conf); /* the runtime whirl parameters, as the cfg left them */
		in.s0.wh.prm = in.whr.cur;
		in.rvG      = e->conf.reverbMix;  /* reverbConfig: setReverbMix */
		in.cabWet   = e->conf.cabMix;     /* convolution.mix */
		in.whBypass = e->conf.bypass;     /* whirlConfig: whirl.bypass */
		/* initWhirl -> computeRotationSpeeds -> setRevSelect(revSelect) ->
		 * useRevOption(revselects[revSelect]), revselects = {4, 0, 8} (src/whirl.cpp:226-293) */
		static const int revselects[3] = {4, 0, 8};
		const int        rs            = revselects[((e->conf.revSelect % 3) + 3) % 3];
		in.revSelect                   = ((e->conf.revSelect % 3) + 3) % 3;
		tbf_wh_state& w  = in.s0.wh;
		w.hornTarget     = e->wt.revHorn[rs];
		w.drumTarget     = e->wt.revDrum[rs];
		w.hornAcDc       = w.hornIncr < w.hornTarget ? 1 : (w.hornTarget < w.hornIncr ? -1 : 0);
		w.drumAcDc       = w.drumIncr < w.drumTarget ? 1 : (w.drumTarget < w.drumIncr ? -1 : 0);
		/* tonegen + vibrato runtime state (initToneGenerator, reset_vibrato) */
		in.s0.mo.keyCompLevel = 1.0f;
		in.s0.mo.percEnvGain  = 0.0f;
		in.s0.tg.outPos       = 1023 / 2;
		in.tg.init (e->tpls[in.tpl].get (), e->conf);
		if (e->slabLen == 0) {
			e->slabLen  = in.k.slabLen;
			e->rvLdsFit = tbf_rv_lds_fits (&in.k) != 0; /* same geometry for every instance */
		} else if (e->slabLen != in.k.slabLen)
			return fail (-22, "inconsistent reverb geometry");
	}
	e->deviceReady = false;
	e->actAll      = true;
	return 0;
}

uint32_t tbf_instance_count (const tbf_engine* e) { return e ? (uint32_t)e->inst.size () : 0; }

int tbf_instance_retune (tbf_engine* e, uint32_t i, uint32_t tpl_id)
{
	if (!e || i >= e->inst.size ())
		return fail (-22, "bad instance");
	if (tpl_id >= e->tpls.size ())
		return fail (-22, "bad template id");
	Instance&          in         = e->inst[i];
	const unsigned int newRouting = in.tg.newRouting;
	/* reinitToneGen (src/clap.cpp:129-157): allocTonegen + initToneGenerator + init_vibrato
	 * on the new tables ... */
	in.tpl   = tpl_id;
	in.k.tpl = tpl_id;
	in.tg.init (e->tpls[tpl_id].get (), e->conf);
	/* ... setToneGenParam (108-121) for the drawbars, vibrato switch and type from the
	 * parameter values (float) ... */
	for (int b = 0; b < 9; b++)
		in.tg.setDrawBar (b, (unsigned)rintf ((float)in.params[TBF_P_DRAWBAR_MIN + b]));
	in.tg.setVibratoUpper ((int)rintf ((float)in.params[TBF_P_VIBRATO]));
	in.tg.setVibratoFromInt ((int)floorf ((float)in.params[TBF_P_VIBRATO_TYPE]));
	/* ... and the routing word kept */
	in.tg.newRouting = newRouting;
	/* the device side: the instance's tone-generator + scanner state (wheel positions, key
	 * compression, percussion envelope and high-pass, stator, scanner ring) starts fresh
	 * at the next block; the preamp fields of tbf_mo_state, reverb and whirl go on */
	tbf_tg_state& g = in.s0.tg;
	memset (&g, 0, sizeof (g));
	g.outPos                = 1023 / 2;
	in.s0.mo.keyCompLevel = 1.0f;
	in.s0.mo.percEnvGain  = 0.0f;
	if (std::find (e->retuned.begin (), e->retuned.end (), i) == e->retuned.end ())
		e->retuned.push_back (i);
	in.progDirty = in.ctlDirty = true;
	markActive (e, i);
	return 0;
}

int tbf_note (tbf_engine* e, uint32_t i, int32_t key, int32_t on)
{
	if (!e || i >= e->inst.size ())
		return fail (-22, "bad instance");
	if (key < 0 || key >= 384)
		return 0; /* oscKeyOn/Off ignore keys >= MAX_KEYS */
	if (on)
		e->inst[i].tg.keyOn (key);
	else
		e->inst[i].tg.keyOff (key);
	markActive (e, i);
	return 0;
}

int tbf_set_param (tbf_engine* e, uint32_t i, int32_t index, double v)
{
	if (!e || i >= e->inst.size ())
		return fail (-22, "bad instance");
	markActive (e, i);
	if (!setParam (e->inst[i], index, (float)v)) /* csrc/tbf_hostctl.cpp */
		return fail (-22, "unknown parameter id");
	e->inst[i].ctlDirty = true;
	return 0;
}

int tbf_config_set (tbf_engine* e, const char* key, const char* value)
{
	if (!e || !key || !value)
		return fail (-22, "null argument");
	Config c     = e->conf;
	int    scope = 0;
	int    rc    = configSet (c, key, value, &scope);
	if (rc == -1)
		return fail (-22, std::string ("bad value for ") + key + ": " + value);
	if (rc == 0)
		return 1; /* not a key of the hot path: ignored, as the reference ignores it */
	if ((scope & CFG_SHARED) && (e->everAdded || !e->inst.empty ()))
		return fail (-16, std::string (key) + " shapes the engine-wide tables: set it before tbf_instances_add");
	const Config old = e->conf;
	e->conf          = c;
	if (scope & CFG_SHARED) {
		if (int r = buildShared (e)) {
			e->conf = old;
			(void)buildShared (e);
			return r;
		}
		e->deviceReady = false;
	}
	return 0;
}

int tbf_config_parse (tbf_engine* e, const char* text)
{
	if (!e || !text)
		return fail (-22, "null argument");
	/* parseConfigurationLine (src/cfgParser.cpp:94-160): `name = value`, '#' comments,
	 * surrounding blanks trimmed.  All or nothing: every line is validated into a copy of
	 * the configuration first, and the copy replaces the engine's only when all pass, so
	 * a caller that gets an error knows that no key took effect. */
	Config      c       = e->conf;
	int         applied = 0, line = 0, scope = 0;
	std::string sharedKey;
	const char* p = text;
	while (*p) {
		const char* q = p;
		while (*q && *q != '\n')
			q++;
		std::string ln (p, q);
		p = *q ? q + 1 : q;
		line++;
		const size_t h = ln.find ('#');
		if (h != std::string::npos)
			ln.resize (h);
		const size_t eq = ln.find ('=');
		auto trim = [] (std::string s) {
			const size_t a = s.find_first_not_of (" \t\r"), b = s.find_last_not_of (" \t\r");
			return a == std::string::npos ? std::string () : s.substr (a, b - a + 1);
		};
		if (trim (ln).empty ())
			continue;
		if (eq == std::string::npos)
			return fail (-22, "line " + std::to_string (line) + ": expected name=value (nothing applied)");
		const std::string k = trim (ln.substr (0, eq)), v = trim (ln.substr (eq + 1));
		int               sc = 0;
		const int         rc = configSet (c, k.c_str (), v.c_str (), &sc);
		if (rc == -1)
			return fail (-22, "line " + std::to_string (line) + ": bad value for " + k + ": " + v + " (nothing applied)");
		if (rc == 0)
			continue; /* not a key of the hot path: ignored, as the reference ignores it */
		if ((sc & CFG_SHARED) && sharedKey.empty ())
			sharedKey = k;
		scope |= sc;
		applied++;
	}
	if ((scope & CFG_SHARED) && (e->everAdded || !e->inst.empty ()))
		return fail (-16, sharedKey + " shapes the engine-wide tables: set it before tbf_instances_add (nothing applied)");
	const Config old = e->conf;
	e->conf          = c;
	if (scope & CFG_SHARED) {
		if (int r = buildShared (e)) {
			e->conf = old;
			(void)buildShared (e);
			return r;
		}
		e->deviceReady = false;
	}
	return applied;
}

} /* extern "C" */

/* ------------------------------------------------------------------ device setup */
/* launch the k_whirl that renderImpl holds back (tbf_engine.defPending), if any */
static int issueDeferred (tbf_engine* e);

/* wait for all pipelined stage work (before the host touches device buffers) */
static int drainStages (tbf_engine* e)
{
	if (int rc = issueDeferred (e))
		return rc;
	if (!e->stagesBusy)
		return 0;
	for (hipStream_t q : e->gs)
		if (q)
			HIPCHK (hipStreamSynchronize (q));
	e->stagesBusy = false;
	return 0;
}

/* make stream s wait for every pipelined stage launch so far */
static int joinStages (tbf_engine* e, hipStream_t s)
{
	if (int rc = issueDeferred (e))
		return rc;
	if (!e->stagesBusy)
		return 0;
	for (hipStream_t q : e->gs) {
		if (!q)
			continue;
		HIPCHK (hipEventRecord (e->sjoin, q));
		HIPCHK (hipStreamWaitEvent (s, e->sjoin, 0));
	}
	e->stagesBusy = false;
	return 0;
}

/* the device program pool with room for `entries`; the persistent slots of the first
 * `keep` instances are carried over */
static int growProg (tbf_engine* e, size_t entries, uint32_t keep)
{
	if (entries <= e->prog.cap)
		return 0;
	if (e->prog.p) /* rare: let every launch that may read the old pool finish */
		HIPCHK (hipDeviceSynchronize ());
	e->stagesBusy = false;
	DevBuf<tbf_prog_entry> np;
	if (np.ensure (entries + entries / 4))
		return fail (-12, "out of device memory (programs)");
	if (keep && e->prog.p)
		HIPCHK (hipMemcpy (np.p, e->prog.p, PERSIST (keep) * sizeof (tbf_prog_entry), hipMemcpyDeviceToDevice));
	e->prog.release ();
	e->prog = std::move (np);
	return 0;
}

static int ensureDevice (tbf_engine* e)
{
	if (e->deviceReady)
		return 0;
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) cannot render");
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipStreamSynchronize (e->stream));
	if (int rc = drainStages (e))
		return rc;
	const uint32_t n = (uint32_t)e->inst.size ();
	/* wave banks + template descriptors.  On the device each wheel's wave is followed by
	 * its first TBF_BLK samples again, so a block's 128 samples from any position < len
	 * are contiguous (the interpreter's wrap split, src/tonegen.cpp:3376-3402, becomes
	 * plain indexing: len >= 384 > 128, so a block wraps at most once) */
	size_t total = 0;
	for (auto& t : e->tpls)
		for (int w = 1; w <= TBF_NW; w++)
			total += t->len[w] + (t->len[w] ? TBF_BLK : 0);
	if (e->bank.ensure (total) || e->tplDesc.ensure (e->tpls.size ()))
		return fail (-12, "out of device memory (bank)");
	std::vector<tbf_tpl_desc> desc (e->tpls.size ());
	std::vector<float>        ext (total);
	size_t                    o = 0;
	for (size_t q = 0; q < e->tpls.size (); q++) {
		const TgTemplate& t = *e->tpls[q];
		memset (desc[q].off, 0, sizeof (desc[q].off));
		memset (desc[q].len, 0, sizeof (desc[q].len));
		for (int w = 1; w <= TBF_NW; w++) {
			const uint32_t L = t.len[w];
			desc[q].off[w]   = (uint32_t)o;
			desc[q].len[w]   = L;
			if (!L)
				continue;
			const float* src = t.bank.data () + t.off[w];
			std::copy (src, src + L, ext.begin () + o);
			for (uint32_t k = 0; k < TBF_BLK; k++)
				ext[o + L + k] = src[k % L];
			o += L + TBF_BLK;
		}
		memcpy (desc[q].attackEnv, t.attackEnv, sizeof (desc[q].attackEnv));
		memcpy (desc[q].releaseEnv, t.releaseEnv, sizeof (desc[q].releaseEnv));
	}
	HIPCHK (hipMemcpy (e->bank.p, ext.data (), total * sizeof (float), hipMemcpyHostToDevice));
	HIPCHK (hipMemcpy (e->tplDesc.p, desc.data (), desc.size () * sizeof (tbf_tpl_desc), hipMemcpyHostToDevice));
	if (e->devCtl) { /* the templates' play matrices (keyContrib) for k_tgctl */
		std::vector<uint32_t>    off (e->tpls.size () * 385);
		std::vector<tbf_contrib> ent;
		for (size_t q = 0; q < e->tpls.size (); q++)
			for (int k = 0; k <= 384; k++) {
				off[q * 385 + k] = (uint32_t)ent.size ();
				if (k < 384)
					for (const Contrib& c : e->tpls[q]->keyContrib[k])
						ent.push_back ({(uint16_t)c.wheel, (uint16_t)c.bus, c.level});
			}
		e->ctlNw = 1;
		for (const tbf_contrib& c : ent)
			e->ctlNw = std::max<uint32_t> (e->ctlNw, (uint32_t)c.wheel + 1u);
		std::vector<float> kc (e->tpls.size () * 128);
		for (size_t q = 0; q < e->tpls.size (); q++)
			memcpy (kc.data () + q * 128, e->tpls[q]->keyCompTable, 128 * sizeof (float));
		if (e->dkeyComp.ensure (std::max<size_t> (kc.size (), 1)))
			return fail (-12, "out of device memory (key compression tables)");
		if (!kc.empty ())
			HIPCHK (hipMemcpy (e->dkeyComp.p, kc.data (), kc.size () * sizeof (float), hipMemcpyHostToDevice));
		if (e->coff.ensure (off.size ()) || e->contrib.ensure (std::max<size_t> (ent.size (), 1)))
			return fail (-12, "out of device memory (play matrices)");
		HIPCHK (hipMemcpy (e->coff.p, off.data (), off.size () * 4, hipMemcpyHostToDevice));
		if (!ent.empty ())
			HIPCHK (hipMemcpy (e->contrib.p, ent.data (), ent.size () * sizeof (tbf_contrib), hipMemcpyHostToDevice));
	}
	/* shared tables */
	const bool errNew = e->err.p == nullptr; /* the path flags are cumulative from the first allocation */
	if (e->vib.ensure (e->vibTab.size ()) || e->whTab.ensure (4 * (size_t)TBF_WH_TSTRIDE) || e->whBw.ensure (e->wt.bw.size ()) ||
	    e->err.ensure (4))
		return fail (-12, "out of device memory (tables)");
	HIPCHK (hipMemcpy (e->vib.p, e->vibTab.data (), e->vibTab.size () * 4, hipMemcpyHostToDevice));
	{
		/* xorshift32 (src/overdrive.cpp:158-160, src/reverb.cpp:775-783) is linear over
		 * GF(2): state after k steps = XOR over the set bits j of the state of
		 * xorshift^k (1 << j).  Column k of row j holds that image, k = 0 .. 128. */
		std::vector<uint32_t> J (32 * TBF_XS_JUMP + 128 * TBF_XS_JUMP);
		xs_jump_table (J.data (), TBF_XS_JUMP);
		/* followed by its nibble-sliced form [8][16][TBF_XS_JUMP] (xs_nib_table) */
		xs_nib_table (J.data () + 32 * TBF_XS_JUMP, J.data (), TBF_XS_JUMP);
		if (e->xsj.ensure (J.size ()))
			return fail (-12, "out of device memory (tables)");
		HIPCHK (hipMemcpy (e->xsj.p, J.data (), J.size () * 4, hipMemcpyHostToDevice));
	}
	{ /* each displacement table followed by its entry 0, so the kernel reads an entry and
	   * its successor (wrapping at 16384) as one pair */
		std::vector<float> padded (4 * (size_t)TBF_WH_TSTRIDE, 0.0f);
		for (int t = 0; t < 4; t++) {
			std::copy (e->wt.displ.begin () + (size_t)t * 16384, e->wt.displ.begin () + (size_t)(t + 1) * 16384,
			           padded.begin () + (size_t)t * TBF_WH_TSTRIDE);
			padded[(size_t)t * TBF_WH_TSTRIDE + 16384] = e->wt.displ[(size_t)t * 16384];
		}
		HIPCHK (hipMemcpy (e->whTab.p, padded.data (), padded.size () * 4, hipMemcpyHostToDevice));
	}
	HIPCHK (hipMemcpy (e->whBw.p, e->wt.bw.data (), e->wt.bw.size () * 4, hipMemcpyHostToDevice));
	if (errNew)
		HIPCHK (hipMemset (e->err.p, 0, 16));
	/* per-instance buffers: new instances start from their initial state, existing
	 * instances keep their device state */
	const uint32_t old = e->devInst;
	if (n > old) {
		DevBuf<tbf_inst_state> nst;
		DevBuf<float>          nwr;
		DevBuf<double>         nsl;
		if (nst.ensure (n) || nwr.ensure ((size_t)n * 4 * e->wringLen) || nsl.ensure ((size_t)n * e->slabLen))
			return fail (-12, "out of device memory (instances)");
		if (old) {
			HIPCHK (hipMemcpy (nst.p, e->st.p, old * sizeof (tbf_inst_state), hipMemcpyDeviceToDevice));
			HIPCHK (hipMemcpy (nwr.p, e->wring.p, (size_t)old * 4 * e->wringLen * 4, hipMemcpyDeviceToDevice));
			HIPCHK (hipMemcpy (nsl.p, e->rslab.p, (size_t)old * e->slabLen * 8, hipMemcpyDeviceToDevice));
		}
		std::vector<tbf_inst_state> s0 (n - old);
		for (uint32_t i = old; i < n; i++)
			s0[i - old] = e->inst[i].s0;
		HIPCHK (hipMemcpy (nst.p + old, s0.data (), (n - old) * sizeof (tbf_inst_state), hipMemcpyHostToDevice));
		HIPCHK (hipMemset (nwr.p + (size_t)old * 4 * e->wringLen, 0, (size_t)(n - old) * 4 * e->wringLen * 4));
		HIPCHK (hipMemset (nsl.p + (size_t)old * e->slabLen, 0, (size_t)(n - old) * e->slabLen * 8));
		e->st.release ();
		e->wring.release ();
		e->rslab.release ();
		e->st    = std::move (nst);
		e->wring = std::move (nwr);
		e->rslab = std::move (nsl);
		std::vector<tbf_inst_const> k (n);
		for (uint32_t i = 0; i < n; i++)
			k[i] = e->inst[i].k;
		if (e->cst.ensure (n) || e->ctl.ensure (2 * CTL_REGION (n)) || e->ctlIdx.ensure (2 * (size_t)n * TBF_CHUNK))
			return fail (-12, "out of device memory (control)");
		e->ctlVer++; /* both regions' persistent entries need the new pool */
		/* program pool: the existing instances' persistent programs move along (the device
		 * control path keeps them only there); new instances start with empty ones */
		if (int rc = growProg (e, PROG_POOL (n, e->devCtl), old))
			return rc;
		HIPCHK (hipMemset (e->prog.p + PERSIST (old), 0, (PERSIST (n) - PERSIST (old)) * sizeof (tbf_prog_entry)));
		if (e->devCtl) {
			DevBuf<tbf_tgc_state> ng;
			if (ng.ensure (n))
				return fail (-12, "out of device memory (control state)");
			if (old)
				HIPCHK (hipMemcpy (ng.p, e->tgc.p, old * sizeof (tbf_tgc_state), hipMemcpyDeviceToDevice));
			HIPCHK (hipMemset (ng.p + old, 0, (n - old) * sizeof (tbf_tgc_state)));
			e->tgc.release ();
			e->tgc = std::move (ng);
		}
		e->persistStale = true;
		if (int rc = cabinetGrow (e, old, n))
			return rc;
		if (int rc = resampleGrow (e, old, n))
			return rc;
		HIPCHK (hipMemcpy (e->cst.p, k.data (), n * sizeof (tbf_inst_const), hipMemcpyHostToDevice));
		e->hCtl.resize (n);
		e->hProg.resize (PERSIST (n));
		e->pslot.resize (n, 0);
		for (uint32_t i = old; i < n; i++) {
			e->hCtl[i].prog_off = (uint32_t)(PSLOTS * i * SLOT);
			e->hProg[PSLOTS * i * SLOT].wheel = 0xFFFF; /* empty program header */
		}
		e->devInst = n;
	}
	e->deviceReady = true;
	return 0;
}

int tbf::engineDevice (tbf_engine* e) { return ensureDevice (e); }

int tbf::engineDrain (tbf_engine* e)
{
	if (e->cfg.device < 0)
		return 0;
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipStreamSynchronize (e->stream));
	return drainStages (e);
}

/* The inter-stage buffers for a call of nblocks blocks: each holds, per instance, one
 * chunk of stageBlocks blocks -- a power of two from TBF_CHUNK up to steadyChunk, just
 * enough for the longest chunk this call can make, so a caller that renders 64 blocks at a
 * time never pays for longer chunks (n x blocks x 128 x 56 B at the default stage
 * groups: 15 GB at 4096 instances and the default 512-block chunks, 60 GB at 2048, 1.9 GB
 * at 64).  They only grow (a different stride under chunks still in flight would be
 * wrong), after every launch that may read them has finished.  When the device cannot hold them, the chunk halves down to
 * TBF_CHUNK before the call fails, and steadyChunk stays at what fitted.  A buffer whose
 * producer and every reader run on one stage-group stream is single: the next chunk's
 * producer is ordered behind this chunk's readers by the stream (default groups {0,0,1,1,1,2}:
 * mid0, rvA and rvB single; mid1, mid2 by chunk parity). */
/* the stage buffers: the stage that writes each, the
 * stages that read it (-1: none; mid0 is read by k_mixpre, mid1 by k_rv_pre and k_rv_post,
 * rvA by k_rv_core, rvB by k_rv_post, mid2 by k_whirl) and its bytes per sample */
enum { SB_MID0, SB_MID1, SB_RVA, SB_RVB, SB_MID2, SB_COUNT };
static const struct StageBuf {
	int    prod, rd[2];
	size_t bytes;
} stageBuf[SB_COUNT] = {{0, {1, -1}, 8}, {1, {2, 4}, 4}, {2, {3, -1}, 16}, {3, {4, -1}, 16}, {4, {5, -1}, 4}};

/* whether buffer b alternates by chunk parity: a reader on another stream than its producer */
static bool stageBufAlternates (const tbf_engine* e, int b)
{
	for (int r : stageBuf[b].rd)
		if (r >= 0 && e->grp[r] != e->grp[stageBuf[b].prod])
			return true;
	return false;
}

/* bytes of the stage buffers at n instances and chunks of `blocks` blocks (each buffer
 * doubled when it alternates by chunk parity) */
static size_t stageFootprint (const tbf_engine* e, size_t n, uint32_t blocks)
{
	const bool rv = chainReverb (e->cfg.chain_mode), fx = chainFx (e->cfg.chain_mode);
	size_t sum = 0;
	for (int b = fx ? SB_MID1 : SB_MID0; b < SB_COUNT; b++) { /* an effects-only chain has no mid0 */
		if (b > SB_MID0 && !rv)
			break;
		sum += (stageBufAlternates (e, b) ? 2 : 1) * stageBuf[b].bytes;
	}
	return sum * n * blocks * TBF_BLK;
}

static int stageBuffers (tbf_engine* e, uint32_t n, uint32_t nblocks, hipStream_t s)
{
	uint32_t want = TBF_CHUNK;
	while (want < nblocks && want < e->steadyChunk)
		want *= 2;
	want = std::min (want, std::max (e->steadyChunk, (uint32_t)TBF_CHUNK));
	const bool fx = chainFx (e->cfg.chain_mode); /* no mid0: stage 1 reads the caller's rows */
	if (e->stageN == n && e->stageBlocks >= want && (fx || e->mid0.p))
		return 0;
	/* every launch that may read the old buffers: pipelined stages and the caller's stream
	 * (the engine's own streams and s; no device-wide synchronization, which would also
	 * wait for a caller's unrelated work on other streams) */
	if (int rc = drainStages (e))
		return rc;
	HIPCHK (hipStreamSynchronize (s));
	const bool rv = chainReverb (e->cfg.chain_mode);
	/* buffer b's elements of `elem` bytes per sample */
	auto       k  = [&] (int b, size_t elem) { return (size_t)(stageBufAlternates (e, b) ? 2 : 1) * (stageBuf[b].bytes / elem); };
	for (uint32_t blocks = want;;) {
		e->mid0.release (), e->mid1.release (), e->mid2.release (), e->rvA.release (), e->rvB.release ();
		const size_t need = (size_t)n * blocks * TBF_BLK;
		const bool   ok   = (fx || !e->mid0.ensure (k (SB_MID0, sizeof (float)) * need)) &&
		                (!rv || (!e->mid1.ensure (k (SB_MID1, sizeof (float)) * need) &&
		                         !e->mid2.ensure (k (SB_MID2, sizeof (float)) * need) &&
		                         !e->rvA.ensure (k (SB_RVA, sizeof (double)) * need) &&
		                         !e->rvB.ensure (k (SB_RVB, sizeof (double)) * need)));
		if (ok) {
			e->stageBlocks = blocks;
			e->stageN      = n;
			if (blocks < want) /* the device could not hold longer chunks */
				e->steadyChunk = blocks;
			return 0;
		}
		(void)hipGetLastError (); /* the failed hipMalloc's error */
		if (blocks <= TBF_CHUNK) {
			e->mid0.release (), e->mid1.release (), e->mid2.release (), e->rvA.release (), e->rvB.release ();
			e->stageBlocks = e->stageN = 0;
			return fail (-12, "out of device memory (stage buffers)");
		}
		blocks = std::max (blocks / 2, (uint32_t)TBF_CHUNK);
	}
}

/* tbf_launch_stage, and the count of the kernel variant it picks (tbf_debug_launches): the
 * same fields it switches on, read here on the host */
static int launchStage (tbf_engine* e, const tbf_launch& P, int k, hipStream_t s)
{
	const int rc = tbf_launch_stage (&P, k, s);
	if (rc || P.nInst == 0 || P.nBlocks == 0)
		return rc;
	if (k == 0)
		e->launches[P.tgSplit > 1 && !P.ctlIdx ? TBF_LAUNCH_TONEGEN_RANGES : TBF_LAUNCH_TONEGEN]++;
	else if (k == 3)
		e->launches[P.rvLds && P.nBlocks >= RVL_MIN_BLOCKS ? TBF_LAUNCH_RV_CORE_LDS : TBF_LAUNCH_RV_CORE]++;
	else if (k == 5)
		e->launches[P.whSplit ? TBF_LAUNCH_WHIRL_SPLIT : TBF_LAUNCH_WHIRL]++;
	return rc;
}

/* one stage launch on stream sk, between the optional timing events (tbf_debug_kernel_times) */
static int timedLaunch (tbf_engine* e, const tbf_launch& P, int k, hipStream_t sk)
{
	hipEvent_t e0 = nullptr, e1 = nullptr;
	if (e->timeOn) {
		HIPCHK (hipEventCreate (&e0));
		HIPCHK (hipEventCreate (&e1));
		HIPCHK (hipEventRecord (e0, sk));
	}
	const int rc = launchStage (e, P, k, sk);
	if (rc)
		return fail (rc, std::string ("kernel launch failed: ") + hipGetErrorString (hipGetLastError ()));
	if (e->timeOn) {
		HIPCHK (hipEventRecord (e1, sk));
		e->tev.push_back ({k, {e0, e1}});
	}
	return 0;
}

/* one pipelined stage launch on its stream, then the events that later stages and chunks
 * wait for */
static int issueStage (tbf_engine* e, const tbf_launch& P, int k, hipStream_t sk, uint64_t cix)
{
	if (int rc = timedLaunch (e, P, k, sk))
		return rc;
	HIPCHK (hipEventRecord (e->sdone[k], sk));
	HIPCHK (hipEventRecord (e->pev[cix & 3][k], sk));
	return 0;
}

/* The held-back k_whirl (k_rv_pre ahead): behind its chunk's k_rv_post, whose event sdone[4]
 * still holds (the next chunk has issued no stage past 2), and behind the caller's stream
 * when it is the call's first output stage.  Nothing has waited for its events yet: every
 * such wait (the stage streams' joins, the buffer-parity waits of the chunk after next, the
 * end of the call) issues it first. */
static int issueDeferred (tbf_engine* e)
{
	if (!e->defPending)
		return 0;
	e->defPending  = false;
	hipStream_t sk = e->gs[e->grp[TBF_NSTAGES - 1]];
	if (!e->outWait) {
		HIPCHK (hipEventRecord (e->sjoin, e->callS));
		HIPCHK (hipStreamWaitEvent (sk, e->sjoin, 0));
		e->outWait = true;
	}
	HIPCHK (hipStreamWaitEvent (sk, e->sdone[TBF_NSTAGES - 2], 0));
	return issueStage (e, e->defP, TBF_NSTAGES - 1, sk, e->defCix);
}

/* The phases of renderBody, in its order (n: the instances; s: the caller's stream; P: the
 * call's launch parameters, whose per-chunk fields the phases fill). */
/* retuned instances (tbf_instance_retune): fresh tone-generator state and the new
 * template id, after every launch so far, before this call's first block */
static int resetRetuned (tbf_engine* e, hipStream_t s)
{
	if (int rc = joinStages (e, s))
		return rc;
	for (uint32_t i : e->retuned) {
		HIPCHK (hipMemcpyAsync (&e->st.p[i].mo, &e->inst[i].s0.mo, offsetof (tbf_mo_state, iirA),
		                        hipMemcpyHostToDevice, s));
		HIPCHK (hipMemcpyAsync (&e->st.p[i].tg, &e->inst[i].s0.tg, sizeof (tbf_tg_state),
		                        hipMemcpyHostToDevice, s));
		HIPCHK (hipMemcpyAsync (&e->cst.p[i].tpl, &e->inst[i].k.tpl, sizeof (uint32_t), hipMemcpyHostToDevice, s));
		if (e->devCtl) { /* a fresh per-wheel control state and an empty program */
			HIPCHK (hipMemsetAsync (e->tgc.p + i, 0, sizeof (tbf_tgc_state), s));
			HIPCHK (hipMemsetAsync (e->prog.p + PSLOTS * i * SLOT, 0, PSLOTS * SLOT * sizeof (tbf_prog_entry), s));
			e->pslot[i]         = 0;
			e->hCtl[i].prog_off = (uint32_t)(PSLOTS * i * SLOT);
			e->persistStale     = true;
		}
	}
	HIPCHK (hipStreamSynchronize (s));
	e->retuned.clear ();
	return 0;
}

/* the launch fields that hold for the whole call */
static int fillLaunch (tbf_engine* e, tbf_launch& P, uint32_t n, float* dL, float* dR, uint64_t stride)
{
	memset (&P, 0, sizeof (P));
	P.bank      = e->bank.p;
	P.tpls      = e->tplDesc.p;
	P.cst       = e->cst.p;
	P.st        = e->st.p;
	P.wring     = e->wring.p;
	P.rslab     = e->rslab.p;
	P.ctl       = e->ctl.p;
	P.vibTab    = e->vib.p;
	P.xsJump    = e->xsj.p;
	P.whTab     = e->whTab.p;
	P.whBw      = e->whBw.p;
	P.outL      = dL;
	P.outR      = dR;
	P.outStride = stride;
	P.nInst     = n;
	P.wringLen  = e->wringLen;
	P.statorInc = e->statorInc;
	P.chain     = tbf_chain_kernels (e->cfg.chain_mode);
	P.ext       = e->extIn;
	P.extStride = e->extStride;
	for (int k = 0; k < 4; k++)
		P.rot[k] = e->rotOut[k];
	P.rotStride = e->rotStride;
	P.whOut     = e->cfg.whirl_out;
	P.slabLen   = e->slabLen;
	P.errFlags  = e->err.p;
	P.dbg       = e->cfg.debug_flags;
	/* k_whirl_split where it keeps more waves per SIMD than k_whirl (tbf_render.hip) */
	P.whSplit = e->whSplit >= 0 ? (uint32_t)e->whSplit : (e->wringLen > 512 || n <= e->nCU) ? 1u : 0u;
	P.rvLds     = e->rvLdsOn && e->rvLdsFit;
	P.rvGrid    = e->rvGrid;
	P.rvWork    = e->rvWork.p;
	if (e->cfg.chain_mode == TBF_CHAIN_TONEGEN && e->mixFixed.ensure (n))
		return fail (-12, "out of device memory");
	P.mixFixed = e->mixFixed.p;
	return 0;
}

/* the blocks of the chunk at b0: TBF_CHUNK at the most, or a steady chunk */
static uint32_t chunkLength (const tbf_engine* e, uint32_t b0, uint32_t nblocks, uint32_t maxChunk, const tbf_event* ev,
                             uint32_t evi, uint32_t nev)
{
	uint32_t want = std::min<uint32_t> (TBF_CHUNK, nblocks - b0);
	if (nblocks - b0 > TBF_CHUNK && maxChunk > TBF_CHUNK && e->actList.empty () && !e->persistStale) {
		/* no instance's control can change before the next event: a chunk without deltas,
		 * up to steadyChunk blocks (as far as the stage buffers reach), ending at the next
		 * event's block */
		uint32_t w = std::min (maxChunk, nblocks - b0);
		if (evi < nev)
			w = std::min (w, ev[evi].block > b0 ? ev[evi].block - b0 : 0u);
		if (w > TBF_CHUNK)
			want = w;
	}
	return want;
}

/* device control, stage-group pipelining: a delta chunk pipelines like any other; its
 * uploads and k_tgctl go on the first stage group's stream after the chunk before
 * last (the previous user of this control region) has finished every stage (nst stages) */
static int usWait (tbf_engine* e, Chunk& ck, hipStream_t s, int nst)
{
	if (ck.usWaited || !ck.dpipe)
		return 0;
	ck.usWaited = true;
	if (!e->stagesBusy) { /* after the caller's stream (earlier non-pipelined work) */
		HIPCHK (hipEventRecord (e->sjoin, s));
		HIPCHK (hipStreamWaitEvent (ck.us, e->sjoin, 0));
	}
	HIPCHK (hipStreamWaitEvent (ck.us, e->pev[(ck.cix + 2) & 3][nst - 1], 0));
	return 0;
}

/* Before the chunk's host control: the persistent control pool when it is stale (after
 * instances were added or retuned), and under device control the wait for the chunk's
 * staging set and its control region's persistent entries */
static int refreshControlPool (tbf_engine* e, ChunkStaging& cs, Chunk& ck, uint32_t n, hipStream_t s, int nst)
{
	int rc;
	if (e->devCtl && e->persistStale) {
		e->ctlVer++; /* the regions refresh below */
		e->persistStale = false;
	}
	if (e->persistStale) {
		/* the persistent pool (entry i = instance i's current control and programme) as
		 * of the START of this chunk: an instance without a delta at some block renders
		 * that block with entry i, so it must not yet hold a later block's events.
		 * Rare (after instances are added), so it syncs. */
		if ((rc = joinStages (e, s)))
			return rc;
		HIPCHK (hipMemcpyAsync (e->ctl.p, e->hCtl.data (), n * sizeof (tbf_seg_ctl), hipMemcpyHostToDevice, s));
		if (!e->devCtl) /* device control keeps the persistent programs on the device */
			HIPCHK (hipMemcpyAsync (e->prog.p, e->hProg.data (), PERSIST (n) * sizeof (tbf_prog_entry),
			                        hipMemcpyHostToDevice, s));
		HIPCHK (hipStreamSynchronize (s));
		e->persistStale = false;
	}
	if (e->devCtl) {
		/* the set was the chunk before last's (its uploads are done once its event is) */
		const auto w0 = std::chrono::steady_clock::now ();
		HIPCHK (hipEventSynchronize (cs.upEv));
		if (e->dbgPhases)
			fprintf (stderr, "chunk %llu: staging wait %.3f ms\n", (unsigned long long)e->chunkSeq,
			         std::chrono::duration<double, std::milli> (std::chrono::steady_clock::now () - w0).count ());
	}
	if (e->devCtl && e->regionVer[ck.rp] != e->ctlVer) {
		/* this region's persistent entries: the control as of the START of this chunk (an
		 * instance renders its blocks before its first delta with entry i) */
		if (!ck.dpipe && (rc = joinStages (e, s)))
			return rc;
		if ((rc = usWait (e, ck, s, nst)))
			return rc;
		cs.hCtlPin.resize (n);
		memcpy ((void*)cs.hCtlPin.data (), e->hCtl.data (), n * sizeof (tbf_seg_ctl));
		HIPCHK (hipMemcpyAsync (e->ctl.p + ck.rp * CTL_REGION (n), cs.hCtlPin.data (), n * sizeof (tbf_seg_ctl),
		                        hipMemcpyHostToDevice, ck.us));
		e->regionVer[ck.rp] = e->ctlVer;
	}
	return 0;
}

/* a delta chunk's uploads: control deltas, delta programs, index table, whirl sets (P.whSets) */
static int uploadDeltas (tbf_engine* e, ChunkStaging& cs, Chunk& ck, tbf_launch& P, hipStream_t s)
{
	const uint32_t n = P.nInst;
	int            rc;
	if (ck.delta) {
		/* device control: both regions' delta slots, sized once for a delta per
		 * instance and block (growProg synchronizes the device when it grows) */
		if (e->devCtl && (rc = growProg (e, PERSIST (n) + 2 * (size_t)n * TBF_CHUNK * SLOT, n)))
			return rc;
		if ((rc = usWait (e, ck, s, tbf_chain_stages (P.chain))))
			return rc;
		if (!e->devCtl) /* device control: k_tgctl writes the deltas' entries (records + full entries) */
			HIPCHK (hipMemcpyAsync (e->ctl.p + ck.rp * CTL_REGION (n) + n, cs.dCtl.data (),
			                        cs.dCtl.size () * sizeof (tbf_seg_ctl), hipMemcpyHostToDevice, ck.us));
		if (!e->dProg.empty ())
			HIPCHK (hipMemcpyAsync (e->prog.p + PERSIST (n), e->dProg.data (),
			                        e->dProg.size () * sizeof (tbf_prog_entry), hipMemcpyHostToDevice, ck.us));
		if (!ck.dfront) /* (k_front writes the index table) */
			HIPCHK (hipMemcpyAsync (e->ctlIdx.p + (size_t)ck.rp * n * TBF_CHUNK, cs.hIdx.data (),
			                        (size_t)ck.len * n * sizeof (uint32_t), hipMemcpyHostToDevice, ck.us));
	}
	P.whSets = nullptr;
	if (ck.delta && !cs.hWh.empty ()) {
		/* the whirl parameter sets of the chunk's deltas, by region parity like the records */
		if (cs.dwh.cap < cs.hWh.size ())
			HIPCHK (hipDeviceSynchronize ()); /* growing: nothing may still read the old buffer */
		if (cs.dwh.ensure (std::max<size_t> (cs.hWh.size (), 64)))
			return fail (-12, "out of device memory (whirl parameter sets)");
		HIPCHK (hipMemcpyAsync (cs.dwh.p, cs.hWh.data (), cs.hWh.size () * sizeof (tbf_wh_params), hipMemcpyHostToDevice, ck.us));
		P.whSets = cs.dwh.p;
	}
	return 0;
}

/* the chunk's launch fields: stage buffers (`need` samples a set), control region, blocks */
static void chunkLaunch (tbf_engine* e, const Chunk& ck, tbf_launch& P, size_t need)
{
	const uint32_t n = P.nInst, len = ck.len;
	auto at = [&] (int b) { return stageBufAlternates (e, b) ? (size_t)ck.bset * need : (size_t)0; };
	P.mid0 = e->mid0.p ? e->mid0.p + 2 * at (SB_MID0) : nullptr;
	P.mid1 = e->mid1.p ? e->mid1.p + at (SB_MID1) : nullptr;
	P.mid2 = e->mid2.p ? e->mid2.p + at (SB_MID2) : nullptr;
	P.rvA  = e->rvA.p ? e->rvA.p + 2 * at (SB_RVA) : nullptr;
	P.rvB  = e->rvB.p ? e->rvB.p + 2 * at (SB_RVB) : nullptr;
	P.prog      = e->prog.p;
	P.ctl       = e->ctl.p + ck.rp * CTL_REGION (n);
	P.ctlIdx    = ck.delta ? e->ctlIdx.p + (size_t)ck.rp * n * TBF_CHUNK : nullptr;
	P.nBlocks   = len;
	/* k_tonegen block ranges (chunks without deltas) for small batches: about 2048 waves,
	 * ranges of >= 4 blocks (each range after the first renders one warm-up block).  At
	 * 4096 instances a split measured no gain (0.73 ms alone either way: the kernel is
	 * bound by its bank gathers and VALU, not by waves in flight). */
	P.tgSplit = e->tgSplit >= 0 ? (uint32_t)std::max (e->tgSplit, 1)
	                            : std::max (1u, std::min ({8u, 2048u / std::max (n, 1u), len / 4}));
	P.tgSplit = std::min (P.tgSplit, std::max (len, 1u));
	P.outOffset = (uint64_t)ck.b0 * TBF_BLK;
	P.extOffset = (uint64_t)ck.b0 * TBF_BLK;
	P.nCtlInst  = 0;
}

/* device control: the chunk's control kernels on us, ahead of k_tonegen, with their uploads:
 * k_front (a front-end chunk: the records, messages and index table from the key states and
 * events) and k_tgctl (the stepped blocks' programs); then the event that frees the set */
static int controlKernels (tbf_engine* e, ChunkStaging& cs, Chunk& ck, tbf_launch& P)
{
	const uint32_t    n = P.nInst, len = ck.len;
	const bool        dfront = ck.dfront;
	const hipStream_t us     = ck.us;
	int               rc;
	if (e->devCtl && (dfront ? ck.delta : !cs.hDInst.empty ())) {
		/* the device buffers are the staging set's: k_tgctl of the chunk before last (same
		 * stream, or the caller's stream when not pipelined) read the other set */
		const size_t nRec  = dfront ? (size_t)n * len : cs.hRec.size ();
		const size_t nMsg  = dfront ? 2 * (size_t)cs.hFevOff[n] : cs.hMsg.size ();
		const size_t nGain = dfront ? (size_t)e->frontGain : cs.hGain.size ();
		if (cs.drec.cap < nRec || cs.dmsg.cap < nMsg || cs.dctlInst.cap < cs.hDInst.size () || cs.dgain.cap < nGain ||
		    cs.dfull.cap < (dfront ? (size_t)n * len : cs.hFull.size ()))
		{
			if (e->dbgPhases)
				fprintf (stderr, "chunk %llu: control record buffers grow (device sync)\n", (unsigned long long)e->chunkSeq);
			HIPCHK (hipDeviceSynchronize ()); /* growing: nothing may still read the old buffers */
		}
		const size_t nFull = dfront ? (size_t)n * len : cs.hFull.size (); /* k_front writes its effect entries */
		if (cs.drec.ensure (std::max<size_t> (nRec, 1)) || cs.dmsg.ensure (std::max<size_t> (nMsg, 1)) ||
		    cs.dgain.ensure (std::max<size_t> (nGain, 27)) ||
		    cs.dctlInst.ensure (cs.hDInst.size ()) || cs.dfull.ensure (std::max<size_t> (nFull, 1)))
			return fail (-12, "out of device memory (control records)");
		P.rec   = cs.drec.p;
		P.msgs  = cs.dmsg.p;
		P.gains = cs.dgain.p;
		P.fulls = cs.dfull.p;
		if (dfront) {
			if (cs.dfront.cap < n || cs.dfev.cap < cs.hFev.size () || cs.dfval.cap < cs.hFev.size () ||
			    cs.dfoff.cap < (size_t)n + 1 || e->dident.cap < n)
				HIPCHK (hipDeviceSynchronize ()); /* growing: nothing may still read the old buffers */
			if (cs.dfront.ensure (n) || cs.dfev.ensure (cs.hFev.size ()) || cs.dfval.ensure (cs.hFev.size ()) ||
			    cs.dfoff.ensure ((size_t)n + 1) || e->dident.ensure (n))
				return fail (-12, "out of device memory (front end)");
			if (e->hIdent.size () != n) {
				e->hIdent.resize (n);
				for (uint32_t i = 0; i < n; i++)
					e->hIdent[i] = i;
				HIPCHK (hipMemcpy (e->dident.p, e->hIdent.data (), (size_t)n * 4, hipMemcpyHostToDevice));
			}
			HIPCHK (hipMemcpyAsync (cs.dfront.p, cs.hFront.data (), (size_t)n * sizeof (tbf_front_state), hipMemcpyHostToDevice, us));
			HIPCHK (hipMemcpyAsync (cs.dfev.p, cs.hFev.data (), cs.hFev.size () * 4, hipMemcpyHostToDevice, us));
			HIPCHK (hipMemcpyAsync (cs.dfoff.p, cs.hFevOff.data (), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, us));
			HIPCHK (hipMemcpyAsync (cs.dfval.p, cs.hFevVal.data (), cs.hFev.size () * 4, hipMemcpyHostToDevice, us));
			P.front   = cs.dfront.p;
			P.fev     = cs.dfev.p;
			P.fevVal  = cs.dfval.p;
			P.fevOff  = cs.dfoff.p;
			P.keyComp = e->dkeyComp.p;
			if ((rc = tbf_launch_front (&P, us)))
				return fail (rc, std::string ("k_front launch failed: ") + hipGetErrorString (hipGetLastError ()));
		}
		for (const auto& g : e->dSeg) /* the filled segments of hRec (none in a front-end chunk) */
			HIPCHK (hipMemcpyAsync (cs.drec.p + g.first, cs.hRec.data () + g.first,
			                        g.second * sizeof (tbf_tgc_rec), hipMemcpyHostToDevice, us));
		if (!dfront && !cs.hMsg.empty ())
			HIPCHK (hipMemcpyAsync (cs.dmsg.p, cs.hMsg.data (), cs.hMsg.size () * sizeof (uint16_t),
			                        hipMemcpyHostToDevice, us));
		if (!dfront && !cs.hGain.empty ())
			HIPCHK (hipMemcpyAsync (cs.dgain.p, cs.hGain.data (), cs.hGain.size () * sizeof (float),
			                        hipMemcpyHostToDevice, us));
		if (!dfront && !cs.hFull.empty ())
			HIPCHK (hipMemcpyAsync (cs.dfull.p, cs.hFull.data (), cs.hFull.size () * sizeof (tbf_seg_ctl),
			                        hipMemcpyHostToDevice, us));
		if (!dfront)
			HIPCHK (hipMemcpyAsync (cs.dctlInst.p, cs.hDInst.data (), cs.hDInst.size () * 4, hipMemcpyHostToDevice, us));
		P.tgc      = e->tgc.p;
		P.ctlInst  = dfront ? e->dident.p : cs.dctlInst.p;
		P.nCtlInst = dfront ? n : (uint32_t)cs.hDInst.size ();
		P.progBase = (uint32_t)(PERSIST (n) + (size_t)ck.rp * n * TBF_CHUNK * SLOT);
		P.coff     = e->coff.p;
		P.contrib  = e->contrib.p;
		P.ctlNw    = e->ctlNw;
		if ((rc = tbf_launch_tgctl (&P, us)))
			return fail (rc, std::string ("k_tgctl launch failed: ") + hipGetErrorString (hipGetLastError ()));
	}
	if (e->devCtl)
		HIPCHK (hipEventRecord (cs.upEv, us)); /* this parity's staging is free after it */
	if (ck.usWaited && ck.piped) /* the stage streams now follow the uploads on us */
		e->stagesBusy = true;
	return 0;
}

/* The chunk's stage launches (aheadOn: k_rv_pre ahead is possible in this call; more: a
 * chunk follows in it).  Not pipelined: one after another on the caller's stream.
 * Pipelined: every chunk's stage k on stream gs[grp[k]], so a stage runs as soon as this
 * chunk's previous stage and the previous chunk's same stage are done, whatever the later
 * stages of the previous chunk are doing.  A stage buffer of this chunk's parity was last
 * read by the chunk before last: its producer waits for those readers (stageBuf) when they
 * run on another stream. */
static int issueChunk (tbf_engine* e, const Chunk& ck, tbf_launch& P, hipStream_t s, bool aheadOn, bool more)
{
	const int      nst = tbf_chain_stages (P.chain);
	/* an effects-only chain starts at stage 1, which reads the caller's rows */
	const int      st0 = tbf_chain_first_stage (e->cfg.chain_mode);
	int            rc;
	/* k_rv_pre ahead: this chunk's k_rv_pre goes in front of the held-back k_whirl of the
	 * chunk before when neither chunk has control deltas or uploads and this one takes
	 * k_rv_core_lds (a shorter chunk's k_rv_pre is too small to matter); its own k_whirl
	 * is held back when a chunk follows in this call.  Anything else runs as before, behind
	 * the held-back launch. */
	const bool plain = aheadOn && ck.piped && !ck.delta && !ck.usWaited && nst == TBF_NSTAGES;
	const bool ahead = plain && e->defPending && P.rvLds && ck.len >= RVL_MIN_BLOCKS;
	if (!ahead && (rc = issueDeferred (e)))
		return rc;
	if (!ck.piped) {
		for (int k = st0; k < nst; k++)
			if ((rc = timedLaunch (e, P, k, s)))
				return rc;
		return 0;
	}
	auto strm = [&] (int k) { return e->gs[e->grp[k == 2 && ahead ? TBF_NSTAGES - 1 : k]]; };
	for (int k = st0; k < nst; k++) {
		hipStream_t sk = strm (k);
		if (k == nst - 1 && plain && more) { /* held back for the next chunk's k_rv_pre */
			e->defP       = P;
			e->defCix     = ck.cix;
			e->defPending = true;
			break;
		}
		/* after the caller's stream (uploads, earlier chunks).  A generator needs that only
		 * when the stage streams are idle; a stage that reads the caller's input needs it on
		 * every call: the input is complete only where the caller's stream reaches the call
		 * (later chunks of the call follow the first on the stage's stream) */
		if (k == st0 && (!e->stagesBusy || (st0 > 0 && !e->inWait))) {
			HIPCHK (hipEventRecord (e->sjoin, s));
			HIPCHK (hipStreamWaitEvent (sk, e->sjoin, 0));
			e->inWait = true;
		}
		if (k == nst - 1 && !e->outWait) { /* the output stage writes the caller's buffers */
			HIPCHK (hipEventRecord (e->sjoin, s));
			HIPCHK (hipStreamWaitEvent (sk, e->sjoin, 0));
			e->outWait = true;
		}
		if (k > 0 && strm (k - 1) != sk)
			HIPCHK (hipStreamWaitEvent (sk, e->sdone[k - 1], 0));
		if (k == 2 && ahead) {
			/* behind k_rv_core of the chunk before (sdone[3] is still its event): that
			 * puts the launch in the k_rv_post phase, orders it behind that chunk's
			 * k_rv_pre (the stage's state) and keeps rvA a single buffer */
			HIPCHK (hipStreamWaitEvent (sk, e->sdone[3], 0));
		} else
			for (const StageBuf& b : stageBuf) /* the readers of the buffer stage k writes */
				for (int r : b.rd)
					if (b.prod == k && r >= 0 && r < nst && strm (r) != sk)
						HIPCHK (hipStreamWaitEvent (sk, e->pev[(ck.cix + 2) & 3][r], 0));
		P.preAhead = k == 2 && ahead;
		if ((rc = issueStage (e, P, k, sk, ck.cix)))
			return rc;
		if (k == 2 && ahead) {
			e->aheadCount++;
			if ((rc = issueDeferred (e))) /* k_whirl of the chunk before, behind it */
				return rc;
		}
	}
	P.preAhead = 0;
	e->stagesBusy = true;
	return 0;
}

/* after a chunk with control deltas: the instances' final entries become their current
 * (pool 0..n-1) control for the next chunk (one-shots cleared).  Device control: k_tgctl
 * left each stepped instance's last program in its other persistent slot; the regions'
 * persistent entries refresh at the start of the chunks that use them.  Host control:
 * uploaded now, and the staging is reused, so it synchronizes. */
static int endDelta (tbf_engine* e, ChunkStaging& cs, uint32_t n, hipStream_t s)
{
	uint32_t lo = n, hi = 0;
	for (uint32_t i = 0; i < n; i++)
		if (e->chg[i]) {
			e->hCtl[i].whRevOption = -1;
			e->hCtl[i].whSet       = 0;
			/* a one-shot in the chunk's last block left the instance dirty only so that the
			 * next block clears it: the entry it ends with is cleared here already */
			Instance& in = e->inst[i];
			if (in.ctlDirty && !in.progDirty && in.revOpt < 0 && !in.whDirty)
				in.ctlDirty = false;
			lo                     = std::min (lo, i);
			hi                     = std::max (hi, i + 1);
			e->chg[i]              = 0;
		}
	if (e->devCtl) {
		for (uint32_t i : cs.hCtlInst) {
			e->pslot[i]         = (uint8_t)((e->pslot[i] + 1) % PSLOTS);
			e->hCtl[i].prog_off = (uint32_t)((PSLOTS * i + e->pslot[i]) * SLOT);
		}
		e->ctlVer++;
		return 0;
	}
	HIPCHK (hipMemcpyAsync (e->ctl.p, e->hCtl.data (), n * sizeof (tbf_seg_ctl), hipMemcpyHostToDevice, s));
	if (hi > lo)
		HIPCHK (hipMemcpyAsync (e->prog.p + lo * PSLOTS * SLOT, e->hProg.data () + lo * PSLOTS * SLOT,
		                        (size_t)(hi - lo) * PSLOTS * SLOT * sizeof (tbf_prog_entry), hipMemcpyHostToDevice, s));
	HIPCHK (hipStreamSynchronize (s));
	return 0;
}

/* One render call: prepare it, then chunk by chunk plan the chunk (Chunk), run its host
 * control into its staging set, upload, issue, and take the deltas over; then the tail. */
static int renderBody (tbf_engine* e, uint32_t nblocks, float* dL, float* dR, uint64_t stride, hipStream_t s,
                       const tbf_event* ev, uint32_t nev)
{
	int rc = ensureDevice (e);
	if (rc)
		return rc;
	const uint32_t n = (uint32_t)e->inst.size ();
	if (n == 0 || nblocks == 0)
		return 0;
	if (chainFx (e->cfg.chain_mode) && !e->extIn)
		return fail (-5, "internal: an effects-only render without an input");
	if (!e->retuned.empty () && (rc = resetRetuned (e, s)))
		return rc;
	if (stride < (uint64_t)nblocks * TBF_BLK)
		return fail (-22, "stride smaller than nblocks*128");
	if (e->actAll || e->inAct.size () != n) { /* new instances: step every one */
		e->inAct.assign (n, 1);
		e->actList.resize (n);
		for (uint32_t i = 0; i < n; i++)
			e->actList[i] = i;
		e->actAll = false;
	}
	tbf_launch P;
	if ((rc = fillLaunch (e, P, n, dL, dR, stride)))
		return rc;
	/* inter-stage buffers for the longest chunk this call makes: single, or two sets by chunk parity */
	if ((rc = stageBuffers (e, n, nblocks, s)))
		return rc;
	const size_t   need     = (size_t)n * e->stageBlocks * TBF_BLK;
	const uint32_t maxChunk = std::min (e->steadyChunk, e->stageBlocks);
	P.midStride             = (uint64_t)e->stageBlocks * TBF_BLK;
	/* Cross-chunk pipelining.  Every stage is causal and keeps its own state, so stage k
	 * of chunk c depends only on stage k-1 of chunk c and on stage k of chunk c-1, which
	 * runs on the same stage-group stream; the stage buffers alternate by chunk parity.
	 * Used for the full chain; tonegen only, tap modes and a host-control chunk's uploads run on the
	 * caller's stream after joining.  With tbf_debug_kernel_times on, each launch is
	 * bracketed by events on its own stream (durations then include the overlap with the
	 * other streams' kernels). */
	const bool pipe = e->pipeline && P.chain == TBF_CHAIN_FULL && !e->timeSerial;
	/* k_rv_pre ahead (tbf_engine.preAhead): with the default stage groups only */
	static const int defGrp[TBF_NSTAGES] = {0, 0, 1, 1, 1, 2};
	const bool       aheadOn = e->preAhead && pipe && std::equal (defGrp, defGrp + TBF_NSTAGES, e->grp);
	const int        nst     = tbf_chain_stages (P.chain);
	e->chg.assign (n, 0);
	uint32_t b0 = 0, evi = 0;
	while (b0 < nblocks) {
		Chunk ck = {};
		ck.b0    = b0;
		ck.evBeg = evi;
		ck.want  = chunkLength (e, b0, nblocks, maxChunk, ev, evi, nev);
		ck.cix   = e->chunkSeq++;
		ck.bset  = (uint32_t)(ck.cix & 1);
		ck.rp    = e->devCtl ? (int)(ck.cix & 1) : 0;
		ck.dpipe = e->devCtl && pipe;
		ck.us    = ck.dpipe ? e->gs[0] : s;
		ChunkStaging& cs = e->stg[ck.rp];
		if ((rc = refreshControlPool (e, cs, ck, n, s, nst)))
			return rc;
		if ((rc = hostControl (e, cs, ck, n, ev, nev)))
			return rc;
		evi      = ck.evBeg;
		ck.piped = pipe && (!ck.delta || ck.dpipe);
		if (!ck.piped && (rc = joinStages (e, s)))
			return rc;
		if ((rc = uploadDeltas (e, cs, ck, P, s)))
			return rc;
		chunkLaunch (e, ck, P, need);
		if ((rc = controlKernels (e, cs, ck, P)))
			return rc;
		if ((rc = issueChunk (e, ck, P, s, aheadOn, b0 + ck.len < nblocks)))
			return rc;
		if (ck.delta && (rc = endDelta (e, cs, n, s)))
			return rc;
		b0 += ck.len;
	}
	for (; evi < nev; evi++) /* events at or after the last block apply to the next render */
		if ((rc = applyEvent (e, ev[evi])))
			return rc;
	if ((rc = issueDeferred (e)))
		return rc;
	/* the caller's stream waits for the last chunk's output stage (which follows
	 * every earlier stage launch); later chunks keep overlapping from the streams */
	if (e->stagesBusy)
		HIPCHK (hipStreamWaitEvent (s, e->sdone[nst - 1], 0));
	return 0;
}

/* renderBody, and on every way out of it the held-back k_whirl: it never outlives the call */
static int renderImpl (tbf_engine* e, uint32_t nblocks, float* dL, float* dR, uint64_t stride, hipStream_t s,
                       const tbf_event* ev = nullptr, uint32_t nev = 0)
{
	e->callS   = s;
	e->outWait = false;
	e->inWait  = false;
	const int rc = renderBody (e, nblocks, dL, dR, stride, s, ev, nev);
	if (e->defPending) { /* an error return between two chunks */
		(void)issueDeferred (e);
		(void)hipStreamWaitEvent (s, e->sdone[TBF_NSTAGES - 1], 0);
	}
	return rc;
}

/* the tbf_render* calls and tbf_synth_sound on an effects-only engine */
static int noRenderOnFx (const tbf_engine* e)
{
	if (chainFx (e->cfg.chain_mode))
		return fail (-22, "effects-only engine (TBF_CHAIN_FX*) has no tone generator to render: "
		                  "use tbf_process / tbf_process_device / tbf_process_events");
	return 0;
}

/* the checks of the tbf_process* calls (the overlap check compares pointers on the host only) */
static int processArgs (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t inStride, const float* outL,
                        const float* outR, uint64_t stride)
{
	if (!e || !in || !outL || !outR)
		return fail (-22, "null argument");
	if (!chainFx (e->cfg.chain_mode))
		return fail (-22, "tbf_process* needs an effects-only engine (TBF_CHAIN_FX*)");
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) cannot render");
	const uint64_t per = (uint64_t)nblocks * TBF_BLK;
	if (inStride < per)
		return fail (-22, "in_stride smaller than nblocks*128");
	if (stride < per)
		return fail (-22, "stride smaller than nblocks*128");
	const uint64_t n = e->inst.size ();
	if (n && per) { /* [first float, one past the last float) of each range */
		const uintptr_t i0 = (uintptr_t)in, i1 = (uintptr_t)(in + (n - 1) * inStride + per);
		for (const float* o : {outL, outR}) {
			const uintptr_t o0 = (uintptr_t)o, o1 = (uintptr_t)(o + (n - 1) * stride + per);
			if (i0 < o1 && o0 < i1)
				return fail (-22, "input and output ranges overlap");
		}
	}
	return 0;
}

/* renderImpl with the call's input rows (tbf_engine.extIn: set for this call only) */
static int processImpl (tbf_engine* e, uint32_t nblocks, const float* dIn, uint64_t inStride, float* dL, float* dR,
                        uint64_t stride, hipStream_t s, const tbf_event* ev = nullptr, uint32_t nev = 0)
{
	e->extIn     = dIn;
	e->extStride = inStride;
	const int rc = renderImpl (e, nblocks, dL, dR, stride, s, ev, nev);
	e->extIn     = nullptr;
	return rc;
}

static int eventsSorted (const tbf_event* ev, uint32_t nev);

/* The checks of the tbf_*_rotors* calls, all before anything renders or steps (in: the
 * effects-only calls' input rows, NULL for the tbf_render_rotors* calls); pointers are compared
 * on the host only. */
static int rotorArgs (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, bool fx, const float* in,
                      uint64_t inStride, const float* outL, const float* outR, uint64_t stride, const tbf_rotor_out* rot)
{
	if (!e || !rot || !rot->hornL || !rot->hornR || !rot->drumL || !rot->drumR || (fx && !in) || (nev && !ev))
		return fail (-22, "null argument");
	if (!outL != !outR)
		return fail (-22, "outL and outR: both or neither");
	if (!chainWhirl (e->cfg.chain_mode))
		return fail (-22, "rotor outputs need a chain that runs the whirl (TBF_CHAIN_FULL, TBF_CHAIN_FX)");
	if (fx != chainFx (e->cfg.chain_mode))
		return fail (-22, fx ? "tbf_process_rotors* needs an effects-only engine (TBF_CHAIN_FX)"
		                     : "effects-only engine (TBF_CHAIN_FX) has no tone generator to render: use tbf_process_rotors*");
	const uint64_t per = (uint64_t)nblocks * TBF_BLK;
	if (rot->stride < per)
		return fail (-22, "rotors->stride smaller than nblocks*128");
	if (outL && stride < per)
		return fail (-22, "stride smaller than nblocks*128");
	if (fx && inStride < per)
		return fail (-22, "in_stride smaller than nblocks*128");
	const uint64_t n = e->inst.size ();
	if (fx && n && per) { /* [first float, one past the last float) of each range */
		const uintptr_t i0 = (uintptr_t)in, i1 = (uintptr_t)(in + (n - 1) * inStride + per);
		const float*    o[6]  = {outL, outR, rot->hornL, rot->hornR, rot->drumL, rot->drumR};
		for (int k = outL ? 0 : 2; k < 6; k++) {
			const uintptr_t o0 = (uintptr_t)o[k], o1 = (uintptr_t)(o[k] + (n - 1) * (k < 2 ? stride : rot->stride) + per);
			if (i0 < o1 && o0 < i1)
				return fail (-22, "input and output ranges overlap");
		}
	}
	if (int rc = eventsSorted (ev, nev))
		return rc;
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) cannot render");
	return 0;
}

/* renderImpl / processImpl with the call's rotor planes (tbf_engine.rotOut: set for this call
 * only).  Without L / R the kernels' L / R stores go to the horn rows, where each lane's horn
 * stores follow them to the same address (wh_flush, tbf_render.hip): no branch around a store
 * and no buffer to throw away. */
static int rotorImpl (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn, uint64_t inStride,
                      float* dL, float* dR, uint64_t stride, const tbf_rotor_out& rot, hipStream_t s)
{
	float* const planes[4] = {rot.hornL, rot.hornR, rot.drumL, rot.drumR};
	std::copy (planes, planes + 4, e->rotOut);
	e->rotStride = rot.stride;
	if (!dL) {
		dL     = rot.hornL;
		dR     = rot.hornR;
		stride = rot.stride;
	}
	const int rc = dIn ? processImpl (e, nblocks, dIn, inStride, dL, dR, stride, s, ev, nev)
	                   : renderImpl (e, nblocks, dL, dR, stride, s, ev, nev);
	std::fill (e->rotOut, e->rotOut + 4, nullptr);
	return rc;
}

int tbf::rotorRender (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn, uint64_t inStride,
                      const tbf_rotor_out& rot, hipStream_t s)
{
	return rotorImpl (e, nblocks, ev, nev, dIn, inStride, nullptr, nullptr, 0, rot, s);
}

int tbf::eventsInOrder (const tbf_event* ev, uint32_t nev) { return eventsSorted (ev, nev); }

int tbf::plainRender (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn, uint64_t inStride,
                      float* dL, float* dR, uint64_t stride, hipStream_t s)
{
	return dIn ? processImpl (e, nblocks, dIn, inStride, dL, dR, stride, s, ev, nev)
	           : renderImpl (e, nblocks, dL, dR, stride, s, ev, nev);
}

/* the host-buffer rotor calls: stage the planes (and L / R, the input) on the device, render,
 * copy back, as tbf_render and tbf_process do */
static int rotorHost (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t inStride, float* outL, float* outR,
                      uint64_t stride, const tbf_rotor_out* rot)
{
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t n   = (uint32_t)e->inst.size ();
	const size_t   per = (size_t)nblocks * TBF_BLK;
	if (n == 0 || per == 0)
		return 0;
	if (e->rotBuf.ensure (4 * (size_t)n * per) || (in && e->extBuf.ensure ((size_t)n * per)) ||
	    (outL && (e->outL.ensure ((size_t)n * per) || e->outR.ensure ((size_t)n * per))))
		return fail (-12, "out of device memory (rotor outputs)");
	if (in)
		HIPCHK (hipMemcpy2DAsync (e->extBuf.p, per * 4, in, inStride * 4, per * 4, n, hipMemcpyHostToDevice, e->stream));
	const size_t        plane = (size_t)n * per;
	const tbf_rotor_out dev   = {e->rotBuf.p, e->rotBuf.p + plane, e->rotBuf.p + 2 * plane, e->rotBuf.p + 3 * plane, per};
	if (int rc = rotorImpl (e, nblocks, nullptr, 0, in ? e->extBuf.p : nullptr, per, outL ? e->outL.p : nullptr,
	                        outL ? e->outR.p : nullptr, per, dev, e->stream))
		return rc;
	float* const host[4] = {rot->hornL, rot->hornR, rot->drumL, rot->drumR};
	for (int k = 0; k < 4; k++)
		HIPCHK (hipMemcpy2DAsync (host[k], rot->stride * 4, e->rotBuf.p + k * plane, per * 4, per * 4, n, hipMemcpyDeviceToHost,
		                          e->stream));
	if (outL) {
		HIPCHK (hipMemcpy2DAsync (outL, stride * 4, e->outL.p, per * 4, per * 4, n, hipMemcpyDeviceToHost, e->stream));
		HIPCHK (hipMemcpy2DAsync (outR, stride * 4, e->outR.p, per * 4, per * 4, n, hipMemcpyDeviceToHost, e->stream));
	}
	HIPCHK (hipStreamSynchronize (e->stream));
	return 0;
}

/* events sorted by block (in parallel: large event lists) */
static int eventsSorted (const tbf_event* ev, uint32_t nev)
{
	const unsigned    T  = std::max (1u, std::min (hostThreads (), (nev + 32767) / 32768));
	const uint32_t    sg = (nev + T - 1) / T;
	std::vector<char> bad (T, 0);
	parallelFor (T, [&] (uint32_t t) {
		const uint32_t k0 = std::max (1u, std::min (nev, t * sg)), k1 = std::min (nev, (t + 1) * sg);
		for (uint32_t k = k0; k < k1; k++)
			if (ev[k].block < ev[k - 1].block) {
				bad[t] = 1;
				return;
			}
	});
	for (char b : bad)
		if (b)
			return fail (-22, "events must be sorted by block");
	return 0;
}

extern "C" {

int tbf_process_device (tbf_engine* e, uint32_t nblocks, const float* dIn, uint64_t inStride, float* dL, float* dR,
                        uint64_t stride, void* stream)
{
	if (int rc = processArgs (e, nblocks, dIn, inStride, dL, dR, stride))
		return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	return processImpl (e, nblocks, dIn, inStride, dL, dR, stride, stream ? (hipStream_t)stream : e->stream);
}

int tbf_process_events (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn,
                        uint64_t inStride, float* dL, float* dR, uint64_t stride, void* stream)
{
	if (nev && !ev)
		return fail (-22, "null argument");
	if (int rc = processArgs (e, nblocks, dIn, inStride, dL, dR, stride))
		return rc;
	if (int rc = eventsSorted (ev, nev))
		return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	return processImpl (e, nblocks, dIn, inStride, dL, dR, stride, stream ? (hipStream_t)stream : e->stream, ev, nev);
}

int tbf_process (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t inStride, float* outL, float* outR,
                 uint64_t stride)
{
	if (int rc = processArgs (e, nblocks, in, inStride, outL, outR, stride))
		return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t n   = (uint32_t)e->inst.size ();
	const size_t   per = (size_t)nblocks * TBF_BLK;
	if (n == 0 || per == 0)
		return 0;
	if (e->extBuf.ensure ((size_t)n * per) || e->outL.ensure ((size_t)n * per) || e->outR.ensure ((size_t)n * per))
		return fail (-12, "out of device memory (input and outputs)");
	HIPCHK (hipMemcpy2DAsync (e->extBuf.p, per * 4, in, inStride * 4, per * 4, n, hipMemcpyHostToDevice, e->stream));
	if (int rc = processImpl (e, nblocks, e->extBuf.p, per, e->outL.p, e->outR.p, per, e->stream))
		return rc;
	HIPCHK (hipMemcpy2DAsync (outL, stride * 4, e->outL.p, per * 4, per * 4, n, hipMemcpyDeviceToHost, e->stream));
	HIPCHK (hipMemcpy2DAsync (outR, stride * 4, e->outR.p, per * 4, per * 4, n, hipMemcpyDeviceToHost, e->stream));
	HIPCHK (hipStreamSynchronize (e->stream));
	return 0;
}

int tbf_render_rotors (tbf_engine* e, uint32_t nblocks, float* outL, float* outR, uint64_t stride, const tbf_rotor_out* rot)
{
	if (int rc = rotorArgs (e, nblocks, nullptr, 0, false, nullptr, 0, outL, outR, stride, rot))
		return rc;
	return rotorHost (e, nblocks, nullptr, 0, outL, outR, stride, rot);
}

int tbf_render_rotors_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, float* dL, float* dR,
                              uint64_t stride, const tbf_rotor_out* rot, void* stream)
{
	if (int rc = rotorArgs (e, nblocks, ev, nev, false, nullptr, 0, dL, dR, stride, rot))
		return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	return rotorImpl (e, nblocks, ev, nev, nullptr, 0, dL, dR, stride, *rot, stream ? (hipStream_t)stream : e->stream);
}

int tbf_process_rotors (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t inStride, float* outL, float* outR,
                        uint64_t stride, const tbf_rotor_out* rot)
{
	if (int rc = rotorArgs (e, nblocks, nullptr, 0, true, in, inStride, outL, outR, stride, rot))
		return rc;
	return rotorHost (e, nblocks, in, inStride, outL, outR, stride, rot);
}

int tbf_process_rotors_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn,
                               uint64_t inStride, float* dL, float* dR, uint64_t stride, const tbf_rotor_out* rot, void* stream)
{
	if (int rc = rotorArgs (e, nblocks, ev, nev, true, dIn, inStride, dL, dR, stride, rot))
		return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	return rotorImpl (e, nblocks, ev, nev, dIn, inStride, dL, dR, stride, *rot, stream ? (hipStream_t)stream : e->stream);
}

int tbf_render_device (tbf_engine* e, uint32_t nblocks, float* dL, float* dR, uint64_t stride, void* stream)
{
	if (!e || !dL || !dR)
		return fail (-22, "null argument");
	if (int rc = noRenderOnFx (e))
		return rc;
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) cannot render");
	HIPCHK (hipSetDevice (e->cfg.device));
	return renderImpl (e, nblocks, dL, dR, stride, stream ? (hipStream_t)stream : e->stream);
}

int tbf_render_events (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, float* dL, float* dR,
                       uint64_t stride, void* stream)
{
	if (!e || !dL || !dR || (nev && !ev))
		return fail (-22, "null argument");
	if (int rc = noRenderOnFx (e))
		return rc;
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) cannot render");
	if (int rc = eventsSorted (ev, nev))
		return rc;
	HIPCHK (hipSetDevice (e->cfg.device));
	return renderImpl (e, nblocks, dL, dR, stride, stream ? (hipStream_t)stream : e->stream, ev, nev);
}

int tbf_render (tbf_engine* e, uint32_t nblocks, float* outL, float* outR, uint64_t stride)
{
	if (!e || !outL || !outR)
		return fail (-22, "null argument");
	if (int rc = noRenderOnFx (e))
		return rc;
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) cannot render");
	HIPCHK (hipSetDevice (e->cfg.device));
	const uint32_t n   = (uint32_t)e->inst.size ();
	const size_t   per = (size_t)nblocks * TBF_BLK;
	if (stride < per)
		return fail (-22, "stride smaller than nblocks*128");
	if (e->outL.ensure ((size_t)n * per) || e->outR.ensure ((size_t)n * per))
		return fail (-12, "out of device memory (outputs)");
	int rc = renderImpl (e, nblocks, e->outL.p, e->outR.p, per, e->stream);
	if (rc || n == 0) /* no instance (all removed): nothing rendered, no row to copy */
		return rc;
	HIPCHK (hipMemcpy2DAsync (outL, stride * 4, e->outL.p, per * 4, per * 4, n, hipMemcpyDeviceToHost, e->stream));
	HIPCHK (hipMemcpy2DAsync (outR, stride * 4, e->outR.p, per * 4, per * 4, n, hipMemcpyDeviceToHost, e->stream));
	HIPCHK (hipStreamSynchronize (e->stream));
	return 0;
}

int tbf_synth_sound (tbf_engine* e, uint32_t nframes, float* outL, float* outR, uint64_t stride)
{
	if (!e || !outL || !outR)
		return fail (-22, "null argument");
	if (int rc = noRenderOnFx (e))
		return rc;
	if (stride < nframes)
		return fail (-22, "stride smaller than nframes");
	const uint32_t n = (uint32_t)e->inst.size ();
	if (n != e->fifoN) {
		/* instances added since the FIFO was filled: they join at the next block (zeros
		 * for the rest of the current one); the others keep their buffered samples */
		std::vector<float> L ((size_t)n * e->fifoLen, 0.f), R ((size_t)n * e->fifoLen, 0.f);
		for (uint32_t i = 0; i < std::min (n, e->fifoN); i++) {
			std::copy_n (e->fifoL.begin () + (size_t)i * e->fifoLen, e->fifoLen, L.begin () + (size_t)i * e->fifoLen);
			std::copy_n (e->fifoR.begin () + (size_t)i * e->fifoLen, e->fifoLen, R.begin () + (size_t)i * e->fifoLen);
		}
		e->fifoL.swap (L);
		e->fifoR.swap (R);
		e->fifoN = n;
	}
	uint32_t written = 0;
	while (written < nframes) {
		if (e->boffset >= e->fifoLen) {
			/* the 128-sample FIFO of synthSound (b_synth/lv2.cpp:1270-1287, src/clap.cpp
			 * PluginRenderAudio) ran dry: render every block this call still needs in one
			 * launch (no event can land between them, so the samples are those of
			 * block-by-block rendering) */
			const uint32_t m = std::min<uint32_t> ((nframes - written + TBF_BLK - 1) / TBF_BLK, 64);
			e->fifoLen       = m * TBF_BLK;
			e->fifoL.resize ((size_t)n * e->fifoLen);
			e->fifoR.resize ((size_t)n * e->fifoLen);
			e->boffset = 0;
			int rc     = tbf_render (e, m, e->fifoL.data (), e->fifoR.data (), e->fifoLen);
			if (rc)
				return rc;
		}
		const uint32_t nread = std::min (nframes - written, e->fifoLen - e->boffset);
		for (uint32_t i = 0; i < n; i++) {
			memcpy (outL + (size_t)i * stride + written, e->fifoL.data () + (size_t)i * e->fifoLen + e->boffset, nread * 4);
			memcpy (outR + (size_t)i * stride + written, e->fifoR.data () + (size_t)i * e->fifoLen + e->boffset, nread * 4);
		}
		written += nread;
		e->boffset += nread;
	}
	return 0;
}

int tbf_synchronize (tbf_engine* e)
{
	if (!e)
		return fail (-22, "null argument");
	if (e->cfg.device < 0)
		return 0;
	HIPCHK (hipSetDevice (e->cfg.device));
	HIPCHK (hipStreamSynchronize (e->stream));
	return drainStages (e);
}

int tbf_error_flags (tbf_engine* e, uint32_t* flags)
{
	if (!e || !flags)
		return fail (-22, "null argument");
	*flags = 0;
	if (!e->err.p)
		return 0;
	HIPCHK (hipSetDevice (e->cfg.device));
	if (int rc = drainStages (e))
		return rc;
	/* the engine stream carries the non-pipelined chunks: read after them, on it */
	HIPCHK (hipMemcpyAsync (flags, e->err.p, 4, hipMemcpyDeviceToHost, e->stream));
	HIPCHK (hipStreamSynchronize (e->stream));
	return 0;
}

int tbf_debug_contrib (tbf_engine* e, uint32_t tid, int32_t key, int16_t* wheel, int16_t* bus, float* level,
                       uint32_t cap)
{
	if (!e || tid >= e->tpls.size () || key < 0 || key >= 384)
		return fail (-22, "bad argument");
	const auto& v = e->tpls[tid]->keyContrib[key];
	for (uint32_t i = 0; i < v.size () && i < cap; i++) {
		wheel[i] = v[i].wheel;
		bus[i]   = v[i].bus;
		level[i] = v[i].level;
	}
	return (int)v.size ();
}

int tbf_debug_tables (tbf_engine* e, uint32_t tid, float* attack, float* release, float* keycomp)
{
	if (!e || tid >= e->tpls.size ())
		return fail (-22, "bad argument");
	const TgTemplate& t = *e->tpls[tid];
	if (attack) memcpy (attack, t.attackEnv, sizeof (t.attackEnv));
	if (release) memcpy (release, t.releaseEnv, sizeof (t.releaseEnv));
	if (keycomp) memcpy (keycomp, t.keyCompTable, sizeof (t.keyCompTable));
	return 0;
}

int tbf_debug_device_program (tbf_engine* e, uint32_t i, float* out, uint32_t cap)
{
	if (!e || i >= e->inst.size () || e->cfg.device < 0 || i >= e->hCtl.size ())
		return fail (-22, "bad instance");
	HIPCHK (hipSetDevice (e->cfg.device));
	if (int rc = drainStages (e))
		return rc;
	HIPCHK (hipStreamSynchronize (e->stream));
	HIPCHK (hipDeviceSynchronize ());
	std::vector<tbf_prog_entry> v (SLOT);
	HIPCHK (hipMemcpy (v.data (), e->prog.p + e->hCtl[i].prog_off, SLOT * sizeof (tbf_prog_entry), hipMemcpyDeviceToHost));
	const uint32_t np = std::min<uint32_t> (v[0].pad, (uint32_t)SLOT - 1);
	for (uint32_t q = 0; q < np && q < cap; q++) {
		const tbf_prog_entry& p = v[1 + q];
		float*                o = out + 9 * q;
		o[0] = p.wheel; o[1] = p.env; o[2] = p.row;
		o[3] = p.sg; o[4] = p.pg; o[5] = p.vg; o[6] = p.nsg; o[7] = p.npg; o[8] = p.nvg;
	}
	return (int)np;
}

int tbf_debug_pool_check (uint32_t jobs)
{
	std::vector<std::atomic<int>> hits (64);
	int                           bad = 0;
	for (uint32_t it = 0; it < jobs; it++) {
		const uint32_t n = 1 + (it * 7919u) % 40;
		for (auto& h : hits)
			h.store (0);
		parallelFor (n, [&] (uint32_t t) {
			hits[t].fetch_add (1);
			if ((t & 7) == 0)
				std::this_thread::yield ();
		});
		bool ok = true;
		for (uint32_t i = 0; i < 64; i++)
			ok = ok && hits[i].load () == (i < n ? 1 : 0);
		bad += ok ? 0 : 1;
	}
	return bad;
}

int tbf_debug_host_time (tbf_engine* e, int32_t reset, double* ms, uint64_t* blocks)
{
	if (!e)
		return fail (-22, "null argument");
	if (ms) *ms = (double)e->hostCtlNs * 1e-6;
	if (blocks) *blocks = e->hostCtlBlocks;
	if (reset)
		e->hostCtlNs = e->hostCtlBlocks = 0;
	return 0;
}

int tbf_debug_layout (const tbf_engine* e, uint32_t* wring_len, float* max_ahead, uint32_t* slab_len)
{
	if (!e)
		return fail (-22, "null argument");
	if (wring_len) *wring_len = e->wringLen;
	if (max_ahead) *max_ahead = e->wt.maxAhead;
	if (slab_len) *slab_len = e->slabLen;
	return 0;
}

int tbf_debug_whirl_lead (const tbf_engine* e, float* min_ahead, float* bound)
{
	if (!e)
		return fail (-22, "null argument");
	if (min_ahead) *min_ahead = e->wt.minAhead;
	if (bound) *bound = TBF_WH_MIN_LEAD;
	return 0;
}

int tbf_debug_chunks (const tbf_engine* e, uint32_t* delta_blocks, uint32_t* steady_blocks)
{
	if (!e)
		return fail (-22, "null argument");
	if (delta_blocks) *delta_blocks = TBF_CHUNK;
	if (steady_blocks) *steady_blocks = e->steadyChunk;
	return 0;
}

int tbf_debug_front_chunks (const tbf_engine* e, uint64_t* device_chunks, uint64_t* host_chunks)
{
	if (!e)
		return fail (-22, "null argument");
	if (device_chunks) *device_chunks = e->frontChunks[0];
	if (host_chunks) *host_chunks = e->frontChunks[1];
	return 0;
}

int tbf_debug_launches (const tbf_engine* e, uint64_t* counts, uint32_t cap)
{
	if (!e || (!counts && cap))
		return fail (-22, "null argument");
	for (uint32_t i = 0; i < cap && i < TBF_LAUNCH_KINDS; i++)
		counts[i] = e->launches[i];
	return TBF_LAUNCH_KINDS;
}

int tbf_debug_pre_ahead (const tbf_engine* e, uint64_t* launches)
{
	if (!e || !launches)
		return fail (-22, "null argument");
	*launches = e->aheadCount;
	return 0;
}

int tbf_set_steady_chunk (tbf_engine* e, uint32_t blocks)
{
	if (!e)
		return fail (-22, "null argument");
	if (int rc = issueDeferred (e)) /* (renderImpl leaves none; before the buffers can change) */
		return rc;
	e->steadyChunk = std::min (std::max (blocks, (uint32_t)TBF_CHUNK), (uint32_t)TBF_STEADY_MAX);
	/* clamped here to what the device can hold for the current instances (the stage
	 * buffers' footprint against the free memory plus the buffers held now), so the value
	 * returned is the one renders use; stageBuffers still halves it on an allocation failure */
	const size_t n = e->inst.size ();
	if (e->cfg.device >= 0 && n) {
		size_t freeB = 0, totalB = 0;
		if (hipSetDevice (e->cfg.device) == hipSuccess && hipMemGetInfo (&freeB, &totalB) == hipSuccess) {
			const size_t held = (e->mid0.cap + e->mid1.cap + e->mid2.cap) * sizeof (float) + (e->rvA.cap + e->rvB.cap) * sizeof (double);
			while (e->steadyChunk > TBF_CHUNK && stageFootprint (e, n, e->steadyChunk) > freeB + held)
				e->steadyChunk = std::max (e->steadyChunk / 2, (uint32_t)TBF_CHUNK); /* 100 -> 64, not 50 */
		} else
			(void)hipGetLastError ();
	}
	if (e->stageBlocks > e->steadyChunk)
		e->stageN = 0; /* reallocated (smaller) at the next render */
	return (int)e->steadyChunk;
}

int tbf_debug_reverb_phase (tbf_engine* e, uint32_t i, int32_t ch, int32_t line, double value)
{
	if (!e || i >= e->inst.size () || ch < 0 || ch > 1 || line < 0 || line > 7)
		return fail (-22, "bad arguments");
	e->inst[i].s0.rv.ch[ch].vib[line] = value; /* an instance not on the device yet takes it at upload */
	if (e->deviceReady && i < e->devInst) {
		HIPCHK (hipSetDevice (e->cfg.device));
		if (int rc = drainStages (e))
			return rc;
		HIPCHK (hipStreamSynchronize (e->stream));
		HIPCHK (hipMemcpy (&e->st.p[i].rv.ch[ch].vib[line], &value, sizeof (double), hipMemcpyHostToDevice));
	}
	return 0;
}

int tbf_debug_step (tbf_engine* e, uint32_t i, float* out, uint32_t cap)
{
	if (!e || i >= e->inst.size ())
		return fail (-22, "bad instance");
	if (e->devCtl)
		return fail (-95, "host programs: the per-wheel control runs on the device (TBF_HOST_CONTROL=1 for the host path)");
	Instance& in = e->inst[i];
	tbf_seg_ctl c;
	memset (&c, 0, sizeof (c));
	in.tg.step (in.prog, c);
	in.progDirty = in.ctlDirty = true;
	markActive (e, i);
	for (uint32_t q = 0; q < in.prog.size () && q < cap; q++) {
		const tbf_prog_entry& p = in.prog[q];
		float*                o = out + 9 * q;
		o[0] = p.wheel; o[1] = p.env; o[2] = p.row;
		o[3] = p.sg; o[4] = p.pg; o[5] = p.vg; o[6] = p.nsg; o[7] = p.npg; o[8] = p.nvg;
	}
	return (int)in.prog.size ();
}

int tbf_debug_exact (int32_t op, const double* in, double* out, uint32_t n)
{
	if (!in || !out || op < 0 || op > 5)
		return fail (-22, "bad arguments");
	static std::vector<uint32_t> J;
	if (op == 3 && J.empty ()) { /* the device layout: bit rows, then the nibble-sliced rows */
		J.resize (32 * TBF_XS_JUMP + 128 * TBF_XS_JUMP);
		xs_jump_table (J.data (), TBF_XS_JUMP);
		xs_nib_table (J.data () + 32 * TBF_XS_JUMP, J.data (), TBF_XS_JUMP);
	}
	for (uint32_t i = 0; i < n; i++) {
		const double* a = in + 3 * i;
		double*       o = out + 2 * i;
		o[0] = o[1] = 0.0;
		if (op == 0) {
			double D = 0.0;
			o[0]     = phase_run (a[0], a[1], (int)a[2], D) ? 1.0 : 0.0;
			o[1]     = D;
		} else if (op == 1) {
			o[0] = cnt_adv ((int)a[0], (int)a[1], (int)a[2]);
		} else if (op == 2) {
			o[0] = wrap1 (a[0]);
		} else if (op == 5) {
			GlibcRand j ((unsigned)a[0]), l ((unsigned)a[0]);
			j.discard ((uint64_t)a[1]);
			for (uint64_t q = 0; q < (uint64_t)a[1]; q++)
				l.next ();
			o[0] = j.next ();
			o[1] = l.next ();
		} else if (op == 4) {
			/* op 4: phase_run_cached along a run of 4096 sub-blocks of m steps from v0
			 * (advancing like the kernel) vs phase_run: out = mismatches, cache hits */
			double   v = a[0], cD = 0, cLo = 0, cHi = 0;
			const int m = (int)a[2];
			uint32_t bad = 0, hits = 0;
			for (int s = 0; s < 4096; s++) {
				double    D1 = 0, D2 = 0;
				const double pD = cD;
				const bool ok1 = phase_run (v, a[1], m, D1);
				const bool ok2 = phase_run_cached (v, a[1], m, D2, cD, cLo, cHi);
				hits += (pD > 0 && cD == pD && ok2) ? 1 : 0;
				if (ok1 != ok2 || (ok1 && D1 != D2))
					bad++;
				if (ok1)
					v = v + (double)m * D1;
				else
					for (int q = 0; q < m; q++)
						v += a[1];
			}
			o[0] = bad;
			o[1] = hits;
		} else {
			/* op 3: xorshift jump as the kernels take it (nibble-sliced table, which must
			 * agree with the bit-row form) vs k literal steps from x0 */
			const uint32_t x0 = (uint32_t)a[0];
			const int      k  = (int)a[1];
			if (k < 0 || k >= TBF_XS_JUMP)
				return fail (-22, "jump length out of range");
			uint32_t x = x0;
			for (int q = 0; q < k; q++)
				x = xs_step (x);
			const uint32_t* N = J.data () + 32 * TBF_XS_JUMP;
			uint32_t        r = 0;
			for (int q = 0; q < 8; q++)
				r ^= N[(q * 16 + ((x0 >> (4 * q)) & 15u)) * TBF_XS_JUMP + k];
			if (r != xs_jump_ref (J.data (), TBF_XS_JUMP, x0, k))
				return fail (-5, "nibble-sliced jump differs from the bit-row jump");
			o[0] = r;
			o[1] = x;
		}
	}
	return 0;
}

int tbf_debug_calibrate (int32_t op, void* buf, uint64_t n, void* stream)
{
	if (!buf || op < 0 || op > 12 || n < 16)
		return fail (-22, "bad arguments");
	int rc = tbf_launch_calibrate (op, buf, n, (hipStream_t)stream);
	return rc ? fail (rc, "calibration launch failed") : 0;
}

int tbf_debug_kernel_times (tbf_engine* e, int32_t enable, double* ms6, uint32_t* count6)
{
	if (!e)
		return fail (-22, "null engine");
	if (enable == 1 || enable == 2 || enable == -1) {
		e->timeOn     = enable >= 1;
		e->timeSerial = enable == 2;
		return 0;
	}
	if (e->cfg.device >= 0)
		HIPCHK (hipSetDevice (e->cfg.device));
	double   ms[TBF_NSTAGES] = {0};
	uint32_t cnt[TBF_NSTAGES] = {0};
	for (auto& t : e->tev) {
		HIPCHK (hipEventSynchronize (t.second.second));
		float v = 0.f;
		HIPCHK (hipEventElapsedTime (&v, t.second.first, t.second.second));
		ms[t.first] += v;
		cnt[t.first]++;
		(void)hipEventDestroy (t.second.first);
		(void)hipEventDestroy (t.second.second);
	}
	e->tev.clear ();
	for (int k = 0; k < TBF_NSTAGES; k++) {
		if (ms6) ms6[k] = ms[k];
		if (count6) count6[k] = cnt[k];
	}
	return 0;
}

} /* extern "C" */
