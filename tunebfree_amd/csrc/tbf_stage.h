/*
 * tbf_stage.h -- the host scaffold the plane stages share (cabinet, rate converter, PCM output,
 * mixdown, bus limiter, loudness meter, true-peak meter): HIPCHK, the timer
 * behind the tbf_debug_*_time hooks, the pieces of a long call with their events, the byte spans
 * of the overlap checks, and the argument checks every stage makes.  Host side only: no .hip file
 * includes it.  Free helpers and one small owning type; a stage's state, launch struct and
 * arithmetic stay in its own files.  tools/stage_san.cpp checks the pieces, the spans and the
 * argument checks against restatements.
 */
#ifndef TBF_STAGE_H
#define TBF_STAGE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tbf.h"

extern "C" int tbf_chain_first_stage (uint32_t chain);

namespace tbf {

int fail (int code, const std::string& msg); /* csrc/tbf_engine.cpp: sets tbf_last_error */

#define HIPCHK(x)                                                                        \
	do {                                                                                 \
		hipError_t _e = (x);                                                             \
		if (_e != hipSuccess)                                                            \
			return fail (-5, std::string (#x ": ") + hipGetErrorString (_e));           \
	} while (0)

/* blocks per piece of a call that renders into engine scratch */
#define TBF_STAGE_PIECE 256u

/* an effects-only chain (TBF_CHAIN_FX*): the caller's audio in place of the tone generator's */
inline bool chainFx (uint32_t chain) { return tbf_chain_first_stage (chain) > 0; }

/* the caller's stream, or the engine's own when the caller names none */
inline hipStream_t streamOr (void* stream, hipStream_t own) { return stream ? (hipStream_t)stream : own; }

/* A stage's timing (tbf_debug_*_time): while it is on, every launch set runs between two events on
 * its stream, and the pairs wait here for the next query.  The pairs left go with the timer. */
struct StageTimer {
	bool                                           on = false;
	std::vector<std::pair<hipEvent_t, hipEvent_t>> pairs;

	StageTimer () = default;
	StageTimer& operator= (StageTimer&& o) noexcept /* takes o's pairs (destroys its own) */
	{
		if (this != &o) {
			release ();
			on = o.on;
			pairs.swap (o.pairs);
		}
		return *this;
	}
	~StageTimer () { release (); }
	void release ()
	{
		for (auto& p : pairs) {
			(void)hipEventDestroy (p.first);
			(void)hipEventDestroy (p.second);
		}
		pairs.clear ();
	}

	/* the body of a tbf_debug_*_time call: enable > 0 / < 0 switches the timing on / off; 0 waits
	 * for the pairs, sums them into ms, counts them into launches and destroys them */
	int query (int32_t enable, double* ms, uint64_t* launches)
	{
		if (enable) {
			on = enable > 0;
			return 0;
		}
		double sum = 0.0;
		for (auto& p : pairs) {
			float t = 0.f;
			HIPCHK (hipEventSynchronize (p.second));
			HIPCHK (hipEventElapsedTime (&t, p.first, p.second));
			sum += t;
		}
		if (ms)
			*ms = sum;
		if (launches)
			*launches = pairs.size ();
		release ();
		return 0;
	}

	/* Around one launch set on stream s: begin () before the first launch, end () behind the last.
	 * Both do nothing while the timing is off.  A guard that goes without end (), because a step
	 * between the two failed, destroys the events it created.  tag: the stage's name in the error. */
	class Guard {
		StageTimer& tm;
		hipStream_t s;
		const char* tag;
		hipEvent_t  t0 = nullptr, t1 = nullptr;
		int         bad () const { return fail (-5, std::string (tag) + " timing events: " + hipGetErrorString (hipGetLastError ())); }

	public:
		Guard (StageTimer& tm_, hipStream_t s_, const char* tag_) : tm (tm_), s (s_), tag (tag_) {}
		Guard (const Guard&)            = delete;
		Guard& operator= (const Guard&) = delete;
		~Guard ()
		{
			if (t0)
				(void)hipEventDestroy (t0);
			if (t1)
				(void)hipEventDestroy (t1);
		}
		int begin ()
		{
			if (!tm.on)
				return 0;
			if (hipEventCreate (&t0) != hipSuccess || hipEventCreate (&t1) != hipSuccess || hipEventRecord (t0, s) != hipSuccess)
				return bad ();
			return 0;
		}
		int end ()
		{
			if (!t0)
				return 0;
			if (hipEventRecord (t1, s) != hipSuccess)
				return bad ();
			tm.pairs.push_back ({t0, t1});
			t0 = t1 = nullptr;
			return 0;
		}
	};
};

/* The pieces of a call of nblocks blocks, at most `piece` (> 0) blocks each, with the events
 * [ev, ev + nev) of the call, which are in block order: for (Pieces pc (...); pc.next ();).
 * A piece's events are pe[0 .. npe), their blocks counted from the piece; the last piece takes
 * those at or beyond the call's end too, which apply after it.  pe points into the caller's array
 * for the first piece and for a piece without events, else to a rebased copy that lives until the
 * next piece. */
struct Pieces {
	uint32_t         p0 = 0, len = 0; /* the piece's first block in the call, and its blocks */
	const tbf_event* pe  = nullptr;
	uint32_t         npe = 0;

	Pieces (const tbf_event* ev_, uint32_t nev_, uint32_t nblocks_, uint32_t piece_)
	    : ev (ev_), nev (nev_), nblocks (nblocks_), piece (std::max (piece_, 1u))
	{
	}
	bool next ()
	{
		evi += npe;
		p0 += len;
		if (p0 >= nblocks)
			return false;
		len             = std::min (piece, nblocks - p0);
		const bool last = p0 + len == nblocks;
		uint32_t   evEnd = evi;
		while (evEnd < nev && (last || ev[evEnd].block < p0 + len))
			evEnd++;
		pe  = ev + evi;
		npe = evEnd - evi;
		if (p0 && npe) {
			pev.assign (ev + evi, ev + evEnd);
			for (tbf_event& v : pev)
				v.block -= p0;
			pe = pev.data ();
		}
		return true;
	}

private:
	const tbf_event*       ev;
	uint32_t               nev, nblocks, piece, evi = 0;
	std::vector<tbf_event> pev;
};

/* [a, b) in bytes; empty ranges overlap nothing */
struct Span {
	uintptr_t a, b;
};

/* `rows` rows of rowBytes bytes, strideBytes apart, from p on; empty for a NULL p, no rows or empty rows */
inline Span rowsSpan (const void* p, uint64_t rows, uint64_t strideBytes, uint64_t rowBytes)
{
	const uintptr_t a = (uintptr_t)p;
	return {a, p && rows && rowBytes ? a + (uintptr_t)((rows - 1) * strideBytes + rowBytes) : a};
}

inline bool overlap (Span x, Span y) { return x.a < x.b && y.a < y.b && x.a < y.b && y.a < x.b; }

/* whether any two of the k spans overlap.  The first nIn of them are inputs, which are only read
 * and may alias each other (a mono source as both channels): pairs among those are not looked at. */
inline bool anyOverlap (const Span* s, int k, int nIn = 0)
{
	for (int a = 0; a < k; a++)
		for (int b = std::max (a + 1, nIn); b < k; b++)
			if (overlap (s[a], s[b]))
				return true;
	return false;
}

/* the most frames a row of the call holds: `frames` without counts, else the largest count, none
 * of which may exceed `frames` (-22 names the first that does) */
inline int countsMost (const char* tag, const uint32_t* counts, uint32_t n, uint32_t frames, uint32_t* most)
{
	*most = counts ? 0u : frames;
	for (uint32_t r = 0; counts && r < n; r++) {
		if (counts[r] > frames)
			return fail (-22, std::string (tag) + ": counts[" + std::to_string (r) + "] above frames");
		*most = std::max (*most, counts[r]);
	}
	return 0;
}

/* rows[0 .. n) are rows of nRows (rows NULL: every row, nothing to check); -22 names the first that is not */
inline int checkRows (const char* tag, uint32_t n, const uint32_t* rows, uint32_t nRows)
{
	for (uint32_t k = 0; rows && k < n; k++)
		if (rows[k] >= nRows)
			return fail (-22, std::string (tag) + ": rows[" + std::to_string (k) + "] " + std::to_string (rows[k]) +
			                      " is no row of n_rows " + std::to_string (nRows));
	return 0;
}

/* x's slot in the list that owns it, or the list's end */
template <typename T>
typename std::vector<std::unique_ptr<T>>::iterator slotOf (std::vector<std::unique_ptr<T>>& v, const T* x)
{
	return std::find_if (v.begin (), v.end (), [x] (const std::unique_ptr<T>& p) { return p.get () == x; });
}

/* a host-buffer call's input, n rows of `per` floats inStride apart, into the engine's staging dExt
 * (tbf_engine.extBuf, rows `per` apart) on stream s */
inline int stageHostInput (float* dExt, const float* in, uint64_t inStride, size_t per, uint32_t n, hipStream_t s)
{
	HIPCHK (hipMemcpy2DAsync (dExt, per * 4, in, inStride * 4, per * 4, n, hipMemcpyHostToDevice, s));
	return 0;
}

} // namespace tbf

#endif
