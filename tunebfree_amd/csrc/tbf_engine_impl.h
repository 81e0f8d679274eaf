/*
 * tbf_engine_impl.h -- private engine state shared by the C-ABI translation units
 * (tbf_engine.cpp: construction, device setup, rendering; tbf_hostctl.cpp: a render chunk's
 * host control; tbf_control.cpp: MIDI control functions and programmes; tbf_fork.cpp: clone,
 * save, load, remove).  Not part of the ABI.
 * The render path (tbf_engine.cpp renderBody) is a chunk loop over
 * phase functions (refreshControlPool, hostControl, uploadDeltas, controlKernels, issueChunk,
 * endDelta) of a Chunk and the chunk's staged arrays, ChunkStaging below.  hostControl is
 * tbf_hostctl.cpp's one entry for it; the others are tbf_engine.cpp's own.
 */
#ifndef TBF_ENGINE_IMPL_H
#define TBF_ENGINE_IMPL_H

#include <hip/hip_runtime.h>

#include <stdlib.h>
#include <string.h>

#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <algorithm>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_cabinet.h"
#include "tbf_comp.h"
#include "tbf_eq.h"
#include "tbf_host.h"
#include "tbf_limit.h"
#include "tbf_loud.h"
#include "tbf_mix.h"
#include "tbf_pcm.h"
#include "tbf_resample.h"
#include "tbf_stage.h"
#include "tbf_tpeak.h"
#include "tbf_types.h"

namespace tbf {

/* one programme of the .pgm table (struct _programme, src/program.h:104-140; the
 * fields the engine applies) */
struct Programme {
	uint32_t flags = 0;
	char     name[32] = {0};
	unsigned drawbars[9] = {0}, lowerDrawbars[9] = {0}, pedalDrawbars[9] = {0};
	uint32_t scanner = 0;
	int      percussionEnabled = 0, percussionVolume = 0, percussionSpeed = 0, percussionHarmonic = 0;
	int      overdriveSelect = 0;
	int      rotarySpeedSelect = 0;
	float    reverbMix = 0.f;
	int      keyboardSplitLower = 0, keyboardSplitPedals = 0;
	int      transpose[7] = {0};
};

int  controlById (struct Instance& in, int id, int value); /* tbf_control.cpp */
void setCharacter (struct Instance& in, float v);

} // namespace tbf

namespace tbf {

/* (tbf_instances_clone / _save / _load copy an instance field by field: a new member goes
 * into ioInstance, csrc/tbf_fork.cpp, too; TgControl's into ioTg) */
struct Instance {
	uint32_t       tpl = 0;
	TgControl      tg;
	tbf_inst_const k;
	tbf_inst_state s0;
	tbf_seg_ctl    ctl;
	double         params[64];
	/* preamp (struct b_preamp) */
	int            odClean = 1;
	float          odA = 0.0f, odB = 0.0f, odC = 1.0f, odD = 0.5f;
	struct OdCache { /* the preamp's control fields for these parameters (odCtl) */
		float       A = 0.f, B = 0.f, C = 0.f, D = 0.f;
		int         clean = 0;
		bool        valid = false;
		tbf_seg_ctl ctl;
	} odc;
	/* reverb mix */
	float          rvG = 0.1f;
	float          cabWet = 1.0f; /* convolution.mix: the cabinet convolver's wet share (csrc/tbf_cabinet.cpp) */
	uint64_t       rsPos = 0;     /* the rate converter's P: engine-rate samples it has consumed (csrc/tbf_resample.cpp) */
	int            whBypass = 0;
	int            revOpt = -1;   /* useRevOption (n) pending for the next block */
	int            revSelect = 0; /* whirl revSelect: WHIRL_SLOW after initWhirl (src/whirl.cpp:1131) */
	WhirlRt        whr;           /* the whirl's MIDI-settable fields ... */
	bool           whDirty = false; /* ... changed since the last block's parameter set */
	GlibcRand      ctlRand{1};    /* control-plane rand() stream (randomizeDrawbars) */
	bool           ctlDirty = true;
	bool           progDirty = true;
	std::vector<tbf_prog_entry> prog;
};

/* host staging in pinned memory (pageable memory if no device: host-only engines), so
 * uploads from it are truly asynchronous; the renderer double-buffers these by chunk */
template <typename T>
struct PinnedVec {
	T*     p      = nullptr;
	size_t n      = 0, cap = 0;
	bool   pinned = false;
	PinnedVec ()  = default;
	PinnedVec (const PinnedVec&) = delete;
	PinnedVec& operator= (const PinnedVec&) = delete;
	~PinnedVec () { release (); }
	void release ()
	{
		if (p && pinned)
			(void)hipHostFree (p);
		else
			free (p);
		p   = nullptr;
		n   = cap = 0;
	}
	void reserve (size_t c)
	{
		if (c <= cap)
			return;
		const size_t nc = std::max<size_t> (std::max<size_t> (c, 2 * cap), 1024);
		T*           q  = nullptr;
		bool         pq = hipHostMalloc ((void**)&q, nc * sizeof (T), 0) == hipSuccess;
		if (!pq)
			q = (T*)malloc (nc * sizeof (T));
		if (n)
			memcpy ((void*)q, (const void*)p, n * sizeof (T));
		const size_t keep = n;
		release ();
		p      = q;
		n      = keep;
		cap    = nc;
		pinned = pq;
	}
	void   push_back (const T& v)
	{
		if (n == cap)
			reserve (n + 1);
		p[n++] = v;
	}
	void   resize (size_t m)
	{
		reserve (m);
		n = m;
	}
	void   clear () { n = 0; }
	size_t size () const { return n; }
	bool   empty () const { return n == 0; }
	T*     data () { return p; }
	T*     begin () { return p; }
	T*     end () { return p + n; }
	T&     operator[] (size_t i) { return p[i]; }
};

/* a chunk's event scan (scanChunk, csrc/tbf_hostctl.cpp): instance ranges and event
 * segments of the device front end's partition, with the per-segment counts */
struct ChunkScan {
	unsigned              T = 1, Te = 1; /* instance ranges, event segments */
	uint32_t              per = 1, seg = 0;
	/* the events of segment s for instance range t, in order, as compact records (written by
	 * the scan itself, so the front end never reads the 24-B events again): rec[boff[s (T +
	 * 1) + t] .. boff[s (T + 1) + t + 1]), inside segment s's own part of rec */
	struct Rec {
		uint32_t inst;
		uint32_t bf; /* block in the chunk << 2 | 1: parameter event | 2: value != 0 */
		int32_t  id;
		float    v;
	};
	std::vector<Rec>      rec;
	std::vector<uint32_t> boff;
};

template <typename T>
struct DevBuf {
	T*     p   = nullptr;
	size_t cap = 0;
	DevBuf ()                         = default;
	DevBuf (const DevBuf&)            = delete; /* one owner: the destructor frees */
	DevBuf& operator= (const DevBuf&) = delete;
	DevBuf& operator= (DevBuf&& o) noexcept /* takes o's buffer (frees its own) */
	{
		if (this != &o) {
			release ();
			p     = o.p;
			cap   = o.cap;
			o.p   = nullptr;
			o.cap = 0;
		}
		return *this;
	}
	~DevBuf () { release (); }
	int    ensure (size_t n)
	{
		if (n <= cap)
			return 0;
		if (p)
			(void)hipFree (p);
		p   = nullptr;
		cap = 0;
		if (hipMalloc ((void**)&p, std::max<size_t> (n, 1) * sizeof (T)) != hipSuccess)
			return -12;
		cap = n;
		return 0;
	}
	void release ()
	{
		if (p)
			(void)hipFree (p);
		p   = nullptr;
		cap = 0;
	}
};

/* One chunk's staged control: what the chunk's host control step writes (pinned host
 * arrays), the device buffers they are uploaded to, and the event behind those uploads.
 * tbf_engine holds two, stg[chunk parity] under device control (stg[0] alone under host
 * control): chunk c + 1's host control fills one while chunk c's uploads and kernels still
 * read the other; a set is free again once its upEv is done.  (A new staged array goes in
 * here, host or device side, and nothing else is needed.) */
struct ChunkStaging {
	PinnedVec<tbf_seg_ctl>     dCtl;     /* the chunk's control deltas (pool entries n ..) */
	PinnedVec<uint32_t>        hIdx;     /* pool entry per (block, instance) */
	PinnedVec<tbf_seg_ctl>     hCtlPin;  /* device control: the region's persistent entries, as uploaded */
	PinnedVec<tbf_tgc_rec>     hRec;     /* per delta of the chunk */
	PinnedVec<uint16_t>        hMsg;     /* the chunk's key messages */
	PinnedVec<float>           hGain;    /* the chunk's changed drawbar gains: (bus, gain) pairs */
	PinnedVec<tbf_wh_params>   hWh;      /* the chunk's whirl parameter sets (tbf_seg_ctl.whSet) */
	PinnedVec<uint32_t>        hCtlInst; /* instances with a stepped delta */
	PinnedVec<uint32_t>        hDInst;   /* instances with any delta: k_tgctl's grid */
	PinnedVec<tbf_seg_ctl>     hFull;    /* the chunk's full control entries (tbf_tgc_rec.full) */
	/* device front end (k_front) for note-only chunks: per instance key state at the chunk
	 * start, the instances' note events by instance, their offsets, TBF_FEV_EFFECT events' values */
	PinnedVec<tbf_front_state> hFront;
	PinnedVec<uint32_t>        hFev, hFevOff;
	PinnedVec<float>           hFevVal;
	/* the device side (k_tgctl, k_front: tbf_ctl.hip) */
	DevBuf<tbf_tgc_rec>        drec;
	DevBuf<uint16_t>           dmsg;
	DevBuf<float>              dgain, dfval;
	DevBuf<tbf_wh_params>      dwh;
	DevBuf<uint32_t>           dctlInst, dfev, dfoff;
	DevBuf<tbf_seg_ctl>        dfull;
	DevBuf<tbf_front_state>    dfront;
	hipEvent_t                 upEv = nullptr; /* after the chunk's uploads and control kernels */
};

/* What renderBody decides for one chunk, handed to the phases of the render path beside
 * the chunk's staged arrays, e->stg[rp] (ChunkStaging). */
struct Chunk {
	uint64_t    cix;          /* the chunk's sequence number (tbf_engine.chunkSeq) */
	int         rp;           /* control region and staging set: cix & 1 under device control, else 0 */
	uint32_t    bset;         /* stage-buffer set: cix & 1 */
	uint32_t    b0, want;     /* first block in the call, blocks planned (chunkLength) ... */
	uint32_t    len;          /* ... and stepped: fewer when the host control ends the chunk early */
	uint32_t    evBeg, evEnd; /* its events (block < b0 + want); evBeg moves past those the host control applied */
	bool        delta, dfront; /* it has control deltas; the device front end (k_front) stepped it */
	bool        dpipe, piped; /* device control and pipelining: uploads on us = gs[0]; stages on the group streams */
	hipStream_t us;           /* the stream of the chunk's uploads and control kernels ... */
	bool        usWaited;     /* ... which has waited for the previous user of this region (usWait) */
};

} // namespace tbf

using namespace tbf; /* private header: the engine's own translation units only */

/* program slots (tbf_types.h TBF_PROG_SLOT: header + entries).  The device program pool
 * holds TBF_PROG_PSLOTS persistent slots per instance (the host-controlled path uses the
 * first), then the chunk's delta programs */
#define SLOT ((size_t)TBF_PROG_SLOT)
#define PSLOTS ((size_t)TBF_PROG_PSLOTS)
#define PERSIST(n) ((size_t)(n) * PSLOTS * SLOT)
/* blocks per kernel launch chunk with control deltas: bounds the inter-stage buffers to
 * n_inst x TBF_CHUNK x 128 floats each (134 MB at 4096 instances) */
#ifndef TBF_CHUNK
#define TBF_CHUNK 64
#endif
/* host-controlled path: delta program entries one chunk may add (a chunk ends early when
 * they would not fit); the device-controlled path sizes its delta slots on demand */
#define DPROG_CAP(n) ((size_t)(n) * SLOT * 2 + 4096)
/* control pool region (one per chunk parity on the device-controlled path; the host path
 * uses region 0): n persistent entries + up to one delta per instance and block */
#define CTL_REGION(n) ((size_t)(n) * (TBF_CHUNK + 1))
/* entries of the device program pool as ensureDevice sizes it for n instances (growProg
 * allocates a quarter more): the persistent slots, then the delta slots -- under device
 * control they grow on demand with a delta chunk */
#define PROG_POOL(n, devCtl) (PERSIST (n) + ((devCtl) ? PERSIST (n) : DPROG_CAP (n)))
/* the most host worker threads (hostThreads; scanChunk sizes its per-range stack arrays by it) */
#define TBF_MAX_HOST_THREADS 16u

#define TBF_NSTAGES 6 /* k_tonegen, k_mixpre, k_rv_pre, k_rv_core, k_rv_post, k_whirl */

/* A bus limiter (tbf_limiter_create, csrc/tbf_limit.cpp): its rows' state and the staging of a
 * call's counts.  The state is input only: per row two history buffers of 2 x Hn floats (L, R),
 * of which rows[r].side is the live one; a call reads it, writes the other and flips the side of
 * every row that took frames (k_limit, csrc/tbf_limit.hip).  With a true-peak detector
 * (tbf_limiter_create_tp: oversample 2 or 4, 0 for the plain kind) Hn is limit_tp_history and the
 * launch is k_limit_tp's (csrc/tbf_limit_tp.hip). */
struct tbf_limiter {
	tbf_engine*                eng = nullptr;
	tbf_limiter_config         cfg = {0.0f, 0u, 0u};
	uint32_t                   nRows = 0, Hn = 0;
	uint32_t                   oversample = 0;
	DevBuf<float>              hist;  /* [row][side][channel][Hn] */
	DevBuf<tbf_limit_row>      drows; /* the call's rows on the device */
	std::vector<tbf_limit_row> rows;  /* .side persists, .count is the call's */
	uint64_t                   launches = 0;
	StageTimer                 timer; /* tbf_debug_limit_time: an event pair around every launch set */
};

/* A loudness meter (tbf_loudness_create, csrc/tbf_loud.cpp): per row and channel the two biquads'
 * state, the open hop's sum and position (tbf_loud_chan), and the energies of the row's complete
 * hops.  The host knows every row's position: pos[r] frames since creation or reset. */
struct tbf_loudness {
	tbf_engine*           eng = nullptr;
	tbf_loudness_config   cfg = {0u, 0u};
	uint32_t              nRows = 0, Hp = 0;
	double                c[7] = {0, 0, 0, 0, 0, 0, 0};
	DevBuf<tbf_loud_chan> state;   /* [row][channel] */
	DevBuf<double>        energy;  /* [row][hop][channel], cfg.max_hops hops a row */
	DevBuf<uint32_t>      dcounts; /* the call's counts on the device */
	std::vector<uint32_t> counts;  /* the call's counts */
	std::vector<uint64_t> pos;     /* frames a row has taken */
	hipStream_t           last = nullptr; /* the stream of the meter's last call or reset */
	StageTimer            timer;   /* tbf_debug_loudness_time: an event pair around every launch */
};

/* A true-peak meter (tbf_true_peak_create, csrc/tbf_tpeak.cpp): per row two sides of 2 x 11 floats
 * of history, of which rows[r].side is the live one, and four words of peaks.  A call reads the live
 * side, writes the other and flips the side of every row that took frames (k_tpeak,
 * csrc/tbf_tpeak.hip).  The host knows every row's position: pos[r] frames since creation or reset. */
struct tbf_true_peak {
	tbf_engine*                eng = nullptr;
	tbf_true_peak_config       cfg = {0u, 0u};
	uint32_t                   nRows = 0;
	DevBuf<float>              hist;  /* [row][side][channel][11] */
	DevBuf<uint32_t>           peaks; /* [row]{sample L, sample R, inter L, inter R}: bit patterns of magnitudes */
	DevBuf<tbf_tpeak_row>      drows; /* the call's rows on the device */
	std::vector<tbf_tpeak_row> rows;  /* .side persists, .count is the call's */
	std::vector<uint64_t>      pos;   /* frames a row has taken */
	hipStream_t                last = nullptr; /* the stream of the meter's last call or reset */
	StageTimer                 timer; /* tbf_debug_true_peak_time: an event pair around every launch */
};

/* A bus equaliser (tbf_eq_create, csrc/tbf_eq.cpp): per row the bands in use and their
 * coefficients, on the host (what tbf_eq_set last gave, and tbf_eq_bands reads back) and on the
 * device, and per row, channel and band the two state doubles (k_eq, csrc/tbf_eq.hip). */
struct tbf_eq {
	tbf_engine*           eng = nullptr;
	tbf_eq_config         cfg = {0u, 0u};
	uint32_t              nRows = 0;
	DevBuf<double>        state;   /* [row][channel][max_bands][2] */
	DevBuf<double>        dcoef;   /* [row][max_bands][5] */
	DevBuf<uint32_t>      dnb;     /* [row] */
	DevBuf<uint32_t>      dcounts; /* the call's counts on the device */
	std::vector<double>   coef;    /* dcoef's host copy */
	std::vector<uint32_t> nb;      /* dnb's host copy */
	std::vector<uint32_t> counts;  /* the call's counts */
	StageTimer            timer;   /* tbf_debug_eq_time: an event pair around every launch */
};

/* A bus compressor (tbf_comp_create, csrc/tbf_comp.cpp): the curves and every row's parameters, on
 * the host (what tbf_comp_curve_set and tbf_comp_rows_set last gave, and the getters read back) and
 * on the device, and per row the gain g (k_comp, csrc/tbf_comp.hip). */
struct tbf_comp {
	tbf_engine*               eng = nullptr;
	tbf_comp_config           cfg = {0u};
	uint32_t                  nRows = 0;
	DevBuf<float>             state;   /* [row]: g */
	DevBuf<float>             dcurves; /* [n_curves][TBF_COMP_POINTS] */
	DevBuf<tbf_comp_row>      drows;   /* [row] */
	DevBuf<uint32_t>          dcounts; /* [row]: the call's counts */
	std::vector<float>        curves;  /* dcurves' host copy */
	std::vector<tbf_comp_row> rows;    /* drows' host copy */
	std::vector<float>        ones;    /* nRows times 1.0f: what a reset copies */
	std::vector<uint32_t>     counts;  /* the call's counts */
	StageTimer                timer;   /* tbf_debug_comp_time: an event pair around every launch */
};

struct tbf_engine {
	tbf_engine_config                       cfg;
	Config                                  conf; /* cfg keys (tbf_config_set) for tables built from now on */
	hipStream_t                             stream = nullptr;
	WhirlTables                             wt;
	std::vector<uint32_t>                   vibTab;
	uint32_t                                statorInc = 0;
	uint32_t                                wringLen  = 512;
	std::vector<std::unique_ptr<TgTemplate>> tpls;
	/* fingerprints for tbf_instances_save / _load (csrc/tbf_fork.cpp), 0: not computed yet:
	 * per template (computed once), and of the engine-wide tables (buildShared resets it) */
	std::vector<uint64_t>                   tplFp;
	uint64_t                                engFp = 0;
	std::vector<Instance>                   inst;
	bool                                    everAdded = false; /* an instance was added once: the table-shaping cfg keys stay
	                                                            * refused (-16) even after tbf_instances_remove took the last one */
	std::vector<uint32_t>                   retuned; /* tbf_instance_retune: device state to reset */
	uint64_t                                hostCtlNs = 0, hostCtlBlocks = 0; /* tbf_debug_host_time */
	/* reverb ring layout (identical for all instances: A..F are fixed) */
	uint32_t                                slabLen = 0;
	/* device side */
	bool                                    deviceReady = false;
	uint32_t                                devInst     = 0;
	DevBuf<float>                           bank;
	DevBuf<tbf_tpl_desc>                    tplDesc;
	DevBuf<tbf_inst_const>                  cst;
	DevBuf<tbf_inst_state>                  st;
	DevBuf<float>                           wring;
	DevBuf<double>                          rslab;
	DevBuf<tbf_seg_ctl>                     ctl;
	DevBuf<tbf_prog_entry>                  prog;
	/* device-side tone-generator control (k_tgctl, tbf_ctl.hip) */
	bool                                    devCtl = false;
	DevBuf<tbf_tgc_state>                   tgc;
	DevBuf<uint32_t>                        coff;
	uint32_t                                ctlNw = 1; /* k_tgctl's staged wheels (largest wheel in coff/contrib + 1) */
	DevBuf<tbf_contrib>                     contrib;
	ChunkStaging                            stg[2];   /* the chunks' staged control, by chunk parity */
	std::vector<tbf_seg_ctl>                lastEmit; /* per instance: the last full entry the device holds (parallel front end) */
	std::vector<uint32_t>                   lastProg;    /* per instance: the last delta's prog_off */
	/* device front end (k_front) for note-only chunks (its staging: ChunkStaging) */
	bool                                    frontOn = true; /* TBF_DEVICE_FRONT=0 disables */
	uint32_t                                frontGain = 0;  /* device front end: the chunk's gain-pair floats */
	DevBuf<float>                           dkeyComp;   /* [tpl][128] keyCompTable */
	DevBuf<uint32_t>                        dident;     /* 0 .. n-1: k_tgctl's grid over every instance */
	std::vector<uint32_t>                   hIdent;
	std::vector<uint8_t>                    fclean; /* per instance: no control change pending but notes */
	std::vector<uint8_t>                    pslot;    /* persistent program slot (0..TBF_PROG_PSLOTS-1) per instance */
	/* device control, pipelined delta chunks: the control pool (persistent entries +
	 * deltas), the index table and the control records come in two regions by chunk
	 * parity; region p's persistent entries are refreshed from hCtl when they are older
	 * than its version (ctlVer counts the changes of hCtl) */
	uint64_t                                ctlVer = 1, regionVer[2] = {0, 0};
	int                                     whSplit = -1; /* k_whirl_split: -1 at rings > 512 or <= 1 instance per CU, 0 / 1 (TBF_WHIRL_SPLIT) */
	uint32_t                                nCU     = 256; /* the device's CUs */
	uint32_t                                frontMin = 64; /* events a chunk needs for the device front end (TBF_FRONT_MIN; 64: profiles/r05/s23) */
	bool                                    parCtl = true; /* TBF_HOST_SERIAL=1 steps serially */
	bool                                    dbgPhases = false; /* TBF_DEBUG_HOST_PHASES: the host phases' times on stderr */
	/* A stepper's sink (csrc/tbf_hostctl.cpp): what one instance range's control steps emit
	 * beside the records -- key messages, gain pairs, whirl sets, full entries, the instances
	 * with a stepped delta (ctlInst) and with any (dInst), the delta count nd -- at offsets
	 * within the sink until mergeSinks moves them into the staging.  One per worker, kept
	 * between chunks so the buffers stay allocated; the serial stepper uses the first.  Worker t
	 * writes its records straight into the staging at base_t = (first instance of its range) *
	 * blocks, and dSeg lists the filled segments {base_t, count_t} of hRec to upload. */
	struct alignas (128) ParStep { /* own cache lines: workers bump these per delta */
		std::vector<uint16_t> msgs;
		std::vector<float>    gains;
		std::vector<tbf_wh_params> whs;
		std::vector<uint32_t> act, ctlInst, evs, dInst, eoff, esort, efill;
		std::vector<ChunkScan::Rec> erec; /* a front-end chunk's events of the range, by instance: what the mirror reads */
		std::vector<tbf_seg_ctl> fulls;
		uint32_t              nd = 0;
		uint32_t              nMsg = 0, nGain = 0; /* msgs and gains in use (the vectors are their room) */
		uint32_t              gainLocal = 0; /* device front end: the range's gain-pair floats */
		bool                  fx = false;    /* ... and whether an effect setter stepped an entry */
		int                   rc = 0;
		std::string           err; /* the worker's tbf_last_error text (it is thread-local) */
	};
	/* per-chunk scratch of the host control step, not double-buffered (no upload reads it
	 * past the chunk): the workers' lists and the filled staging segments, the host path's
	 * delta programs, membership of hCtlInst / hDInst, lastEmit taken, control changed, the
	 * pool entry per instance at the current block, the event scan (scanChunk) */
	std::vector<ParStep>                    parStep;
	std::vector<std::pair<uint32_t, uint32_t>> dSeg;
	std::vector<tbf_prog_entry>             dProg;
	std::vector<uint8_t>                    stepped, dhas, dseen, chg;
	std::vector<uint32_t>                   curIdx;
	ChunkScan                               scan;
	DevBuf<uint32_t>                        vib;
	DevBuf<uint32_t>                        xsj; /* xorshift32 jump table */
	DevBuf<float>                           whTab, whBw;
	DevBuf<uint32_t>                        err;
	/* tbf_debug_kernel_times: HIP events around every stage launch */
	bool                                    timeOn = false;
	bool                                    timeSerial = false; /* time with pipelining off */
	std::vector<std::pair<int, std::pair<hipEvent_t, hipEvent_t>>> tev;
	DevBuf<float>                           outL, outR;
	DevBuf<float>                           extBuf; /* tbf_process: the host input on the device */
	/* k_state_move (csrc/tbf_fork.cpp): the packed records of a save / load, and the pair lists */
	DevBuf<unsigned char>                   stStage;
	DevBuf<uint32_t>                        stPairs;
	DevBuf<float>                           mid0, mid1, mid2; /* inter-stage blocks of one launch chunk */
	DevBuf<double>                          rvA, rvB;   /* reverb inter-kernel streams (FP64) */
	std::vector<tbf_seg_ctl>                hCtl;  /* current control per instance (pool entries 0..n-1) */
	std::vector<tbf_prog_entry>             hProg; /* current program per instance (slots i * PROG_CAP) */
	/* instances whose control may change at the next block (renderImpl steps only
	 * these): every entry point that changes an instance marks it (markActive) */
	std::vector<uint32_t>                   actList;
	std::vector<uint8_t>                    inAct;   /* membership of actList */
	bool                                    actAll = true; /* instances added: step all */
	DevBuf<uint32_t>                        ctlIdx;
	bool                                    persistStale = true; /* device pool entries 0..n-1 need upload */
	/* cross-chunk pipelining (renderImpl): stage k of every chunk runs on the stream of its
	 * stage group grp[k] (so the stage's own state is ordered by its stream), the stages of
	 * one chunk are chained by events, and a stage that overwrites a stage buffer of parity
	 * c % 2 waits for chunk c - 2's readers of it on other streams.  A stage therefore starts
	 * as soon as its inputs are ready, whatever the later stages of earlier chunks do.
	 * Three groups: the device exposes few hardware queues per process (GPU_MAX_HW_QUEUES 4)
	 * and streams sharing one serialize. */
	hipStream_t                             gs[TBF_NSTAGES] = {};     /* groups 0 .. grp[TBF_NSTAGES - 1] */
	hipEvent_t                              sdone[TBF_NSTAGES] = {};  /* the last launched chunk's stage k */
	hipEvent_t                              pev[4][TBF_NSTAGES] = {}; /* chunk c's stage k, ring by c mod 4 */
	hipEvent_t                              sjoin = nullptr;
	uint64_t                                chunkSeq = 0;
	bool                                    stagesBusy = false; /* pipelined work may be outstanding */
	bool                                    pipeline = true;    /* TBF_PIPELINE=0 disables */
	/* stage k's stream (TBF_PIPE_GROUPS): k_tonegen + k_mixpre | k_rv_pre + k_rv_core + k_rv_post |
	 * k_whirl.  Against {0,0,1,1,2,2}: rvB single (its producer and reader share a stream),
	 * mid2 by parity, 56 instead of 68 B per stereo sample, and the step 131.7 -> 128.3 ms
	 * (profiles/r05/s20_groups) */
	int                                     grp[TBF_NSTAGES] = {0, 0, 1, 1, 1, 2};
	/* k_rv_pre ahead (TBF_PRE_AHEAD=1; default groups, full chain): chunk c + 1's k_rv_pre runs on
	 * the k_whirl stream in front of k_whirl (c), behind k_mixpre (c + 1) and k_rv_core (c), so it
	 * shares the CUs with k_rv_post (c) and not with k_whirl (c).  Chunks are issued
	 * chunk-major, so k_whirl (c)'s launch is held back (def*) until chunk c + 1 has issued its
	 * stage 2, or until anything else needs the streams complete (issueDeferred: joinStages,
	 * drainStages, the end of the call).  It never outlives renderImpl.  Measured slower than
	 * the default order, so off unless switched on. */
	bool                                    preAhead   = false;
	bool                                    defPending = false;   /* k_whirl of chunk defCix is held back */
	tbf_launch                              defP;                 /* its launch */
	uint64_t                                defCix     = 0;
	hipStream_t                             callS      = nullptr; /* the caller's stream of the current renderImpl ... */
	bool                                    outWait    = false;   /* ... which the output stage has waited for */
	/* effects-only chains (TBF_CHAIN_FX*): the current call's input rows (tbf_process*; NULL in a
	 * tbf_render* call), and whether the call's first stage has waited for the caller's stream
	 * yet: a generator's first stage waits only when the stage streams are idle, a stage that
	 * reads the caller's buffer waits on every call (the input-side analogue of outWait) */
	const float*                            extIn      = nullptr;
	uint64_t                                extStride  = 0;
	/* the current call's rotor planes hornL, hornR, drumL, drumR (tbf_*_rotors*; NULL in every
	 * other call), and the host-buffer variants' staging of the four (plane k at rotBuf + k * n * per) */
	float*                                  rotOut[4]  = {nullptr, nullptr, nullptr, nullptr};
	uint64_t                                rotStride  = 0;
	DevBuf<float>                           rotBuf;
	bool                                    inWait     = false;
	uint64_t                                aheadCount = 0;       /* k_rv_pre launches that ran ahead (tbf_debug_pre_ahead) */
	/* the cabinet convolver (tbf_cabinet_set, csrc/tbf_cabinet.cpp): the engine-wide response and
	 * its tables, the per-instance history st (a k_state_move segment like st / wring / rslab:
	 * 2 * TBF_CAB_CH_FLOATS (K) floats per instance), the mix as the device holds it */
	struct Cabinet {
		uint32_t           taps = 0, K = 0; /* taps 0: no cabinet */
		uint64_t           fp   = 0;        /* fingerprint of the taps (blob header) */
		std::vector<float> ir[2];
		bool               tablesUp = false; /* H and tw are on the device */
		DevBuf<float>      H[2], tw, st, wet0, wetBlk;
		DevBuf<float>      hostOut;          /* the host-buffer calls' staging: wet pair and rotor planes */
		std::vector<float> wetDev;           /* wet0 as uploaded */
		uint64_t           launches = 0;     /* k_cabinet launches (tbf_debug_cabinet) */
		StageTimer         timer;            /* tbf_debug_cabinet_time: an event pair around every launch */
		uint64_t           instFloats () const { return K ? 2 * TBF_CAB_CH_FLOATS (K) : 0; }
	} cab;
	/* the output rate converter (tbf_resampler_set, csrc/tbf_resample.cpp): the engine-wide
	 * prototype and its phase-major table, the per-instance history st (a k_state_move segment
	 * like the cabinet's: 2 * TBF_RS_HIST (T) floats per instance).  The positions are the
	 * instances' (Instance::rsPos) */
	struct Resampler {
		uint32_t           Fo = 0, L = 0, M = 0, T = 0; /* L 0: no converter */
		uint32_t           TO = 0, TS = 0;              /* k_resample's tile: outputs, taps per segment, */
		uint32_t           winFloats = 0, ldsRow = 0;   /* its LDS window and the table's row stride in LDS (0: not there) */
		uint64_t           fp = 0;                      /* fingerprint of the table (blob header) */
		std::vector<float> g, pm;                       /* g[k] as defined; the same phase-major, rows of TBF_RS_ROW (T) */
		bool               tabUp = false;               /* pm is on the device */
		DevBuf<float>      tab, st, hostOut;            /* hostOut: the host-buffer calls' staging of the converted pair */
		DevBuf<uint64_t>   pos;                         /* positions per instance, when they differ */
		uint64_t           launches = 0;
		StageTimer         timer;                       /* tbf_debug_resample_time: an event pair around every launch */
		uint32_t           histFloats () const { return L ? TBF_RS_HIST (T) : 0; }
		uint64_t           instFloats () const { return 2 * (uint64_t)histFloats (); }
	} rs;
	/* the PCM output stage (csrc/tbf_pcm.cpp): no instance state, only the calls' staging -- the
	 * rows' counts and dither frames when they differ, the host-buffer calls' packed rows and meters */
	struct Pcm {
		DevBuf<tbf_pcm_row>   rows;
		DevBuf<unsigned char> hostOut;
		DevBuf<tbf_pcm_meter> hostMeters;
		uint64_t              launches = 0;
		StageTimer            timer;        /* tbf_debug_pcm_time: an event pair around every launch */
	} pcm;
	/* the mixdown stage (csrc/tbf_mix.cpp): no instance state, only the calls' staging -- the
	 * bus-sorted member list and the host-buffer calls' bus planes */
	struct Mix {
		DevBuf<uint32_t>       busOff;
		DevBuf<tbf_mix_member> members;
		DevBuf<float>          hostOut;
		uint64_t               launches = 0;
		StageTimer             timer;        /* tbf_debug_mix_time: an event pair around every launch */
	} mix;
	bool                                    rvLdsOn  = true;  /* k_rv_core_lds when the rings fit (TBF_RV_LDS=0: k_rv_core) */
	bool                                    rvLdsFit = false; /* the instances' rings fit k_rv_core_lds */
	uint32_t                                rvGrid   = 0;     /* k_rv_core_lds persistent workgroups (TBF_RV_PERSIST=0: one per pair) */
	DevBuf<uint32_t>                        rvWork;           /* its work counter */
	DevBuf<uint8_t>                         mixFixed;         /* tonegen only: k_tonegen wrote the output (tbf_launch.mixFixed) */
	int                                     tgSplit  = -1;    /* k_tonegen block ranges (TBF_TG_SPLIT; -1: by batch size) */
	uint32_t                                steadyChunk = TBF_STEADY_DEFAULT; /* blocks per chunk without control deltas (TBF_STEADY_CHUNK,
	                                                                           * tbf_set_steady_chunk) */
	/* the stage buffers as allocated (stageBuffers): blocks per chunk they hold (a power of two
	 * from TBF_CHUNK up to steadyChunk, grown to the longest chunk a call can make, never past
	 * what the device could allocate), for stageN instances; a buffer whose producer and
	 * readers share a stage-group stream is single, the others alternate by chunk parity
	 * (stageBufAlternates) */
	uint32_t                                stageBlocks = 0, stageN = 0;
	uint64_t                                frontChunks[2] = {0, 0}; /* chunks with events: device, host front end */
	/* kernel variants launched (tbf_debug_launches, TBF_LAUNCH_*): k_tonegen with one block
	 * range / several, k_rv_core, k_rv_core_lds, k_whirl, k_whirl_split */
	uint64_t                                launches[6] = {0, 0, 0, 0, 0, 0};
	/* programme table (.pgm), src/program.h:26 MAXPROGS; pgm.controller.offset */
	std::vector<Programme>                  progs = std::vector<Programme> (129);
	int                                     pgmOffset = 1;
	/* synth_sound FIFO */
	std::vector<float>                      fifoL, fifoR;
	uint32_t                                boffset = TBF_BLK; /* read position in the FIFO ... */
	uint32_t                                fifoLen = TBF_BLK; /* ... of fifoLen samples per instance ... */
	uint32_t                                fifoN   = 0;       /* ... for fifoN instances */
	/* the bus limiters still alive (csrc/tbf_limit.cpp); they go with the engine.  Behind every
	 * member the render path reads, so that nothing it reads has moved. */
	std::vector<std::unique_ptr<tbf_limiter>> limiters;
	/* the loudness meters still alive (csrc/tbf_loud.cpp), likewise, and behind the limiters for the
	 * same reason */
	std::vector<std::unique_ptr<tbf_loudness>> loudness;
	/* the true-peak meters still alive (csrc/tbf_tpeak.cpp), likewise, and behind the loudness meters */
	std::vector<std::unique_ptr<tbf_true_peak>> truePeaks;
	/* the bus equalisers still alive (csrc/tbf_eq.cpp), likewise, and behind the true-peak meters */
	std::vector<std::unique_ptr<tbf_eq>> eqs;
	/* the bus compressors still alive (csrc/tbf_comp.cpp), likewise, and behind the equalisers */
	std::vector<std::unique_ptr<tbf_comp>> comps;
};

namespace tbf {
/* csrc/tbf_hostctl.cpp: one chunk's host control into its staging set (renderBody's phase);
 * a scheduled event applied; tbf_set_param's setter.  (tbf_debug_render_program of the
 * debug ABI is defined there too: it makes one stepControl call.) */
int  hostControl (tbf_engine* e, ChunkStaging& cs, Chunk& ck, uint32_t n, const tbf_event* ev, uint32_t nev);
int  applyEvent (tbf_engine* e, const tbf_event& ev);
bool setParam (Instance& in, int32_t index, float value);
/* csrc/tbf_engine.cpp: the host worker pool */
unsigned hostThreads ();
void     parallelFor (uint32_t n, const std::function<void (uint32_t)>& f);
/* the calling thread's active list while renderImpl steps an instance range on a host
 * worker thread (nullptr: the engine's own list) */
extern thread_local std::vector<uint32_t>* tlAct;
/* for csrc/tbf_fork.cpp: the device arrays sized and filled for every instance
 * (ensureDevice), and the wait for the engine's stream and the pipelined stage streams */
int engineDevice (tbf_engine* e);
int engineDrain (tbf_engine* e);
/* for csrc/tbf_cabinet.cpp: one render (dIn NULL) or effects-only pass into the four rotor
 * planes alone, on stream s (rotorImpl without L / R); the events' order check */
int rotorRender (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn, uint64_t inStride,
                 const tbf_rotor_out& rot, hipStream_t s);
int eventsInOrder (const tbf_event* ev, uint32_t nev);
/* csrc/tbf_cabinet.cpp: the history array regrown for n instances (ensureDevice: the first
 * `old` keep theirs, the new ones start from zeros); convolution.mix's value of a control value */
int cabinetGrow (tbf_engine* e, uint32_t old, uint32_t n);
/* for csrc/tbf_resample.cpp: one render (dIn NULL) or effects-only pass into L / R on stream s
 * (renderImpl / processImpl); the converter's history array regrown as cabinetGrow's */
int plainRender (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn, uint64_t inStride,
                 float* dL, float* dR, uint64_t stride, hipStream_t s);
int resampleGrow (tbf_engine* e, uint32_t old, uint32_t n);
inline float cabinetWet (int u) { return (float)((double)(u > 127 ? 127 : u) / 127.0); }
inline void markActive (tbf_engine* e, uint32_t i)
{
	if (i < e->inAct.size () && !e->inAct[i]) {
		e->inAct[i] = 1;
		(tlAct ? *tlAct : e->actList).push_back (i);
	}
}
} // namespace tbf

#endif
