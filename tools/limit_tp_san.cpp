/*
 * tools/limit_tp_san.cpp -- the true-peak limiter's host restatement under AddressSanitizer + UBSan
 * (make -C tunebfree_amd limit_tp_san; a CPU program, no device): tbf_debug_limit_tp_ref and
 * tbf_debug_limit_tp_grid over heap arrays of exactly the sizes the calls are entitled to, so that
 * one element read or written beyond them is reported.  Seeded rows that exceed the ceiling are
 * taken in one call and in cuts at 1, 5, 6, 7, 11, 12, D + 6 and Hn_tp + 3 frames, alone and
 * together, at several (ahead, hold, oversample); outputs, meters and history must be the same
 * bits.  The refusals of a host-only engine's tbf_limiter_create_tp run under the same sanitizers.
 * Exit code 0 and "limit_tp_san: ok" when everything held.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "tbf.h"

static uint32_t lcg (uint32_t& s) { return s = s * 1664525u + 1013904223u; }

#define CHECK(x)                                                                  \
	do {                                                                          \
		if (!(x)) {                                                               \
			fprintf (stderr, "limit_tp_san: %s failed (line %d): %s\n", #x, __LINE__, tbf_last_error ()); \
			return 1;                                                             \
		}                                                                         \
	} while (0)

static int run (uint32_t A, uint32_t H, uint32_t F, uint32_t n)
{
	const tbf_limiter_config cfg = {1.0f - 1.0f / 32768.0f, A, H};
	const tbf_limiter_detect det = {F, 0u};
	std::unique_ptr<uint32_t> group (new uint32_t), tile (new uint32_t), hist (new uint32_t), lds (new uint32_t);
	CHECK (tbf_debug_limit_tp_grid (&cfg, &det, group.get (), tile.get (), hist.get (), lds.get ()) == 0);
	CHECK (tbf_debug_limit_tp_grid (&cfg, &det, nullptr, nullptr, nullptr, nullptr) == 0);
	const uint32_t Hn = *hist, D = A - 1u;
	CHECK (Hn == 2u * A + H + 9u && *lds <= 160u * 1024u && *tile % (64u * *group) == 0u);

	std::unique_ptr<float[]> L (new float[n]), R (new float[n]);
	uint32_t                 seed = A * 31u + H * 7u + F + n;
	for (uint32_t i = 0; i < n; i++) { /* noise of amplitude 0.5 with a burst of 3 every 97 frames */
		const float s = i % 97u < 3u ? 3.0f : 0.5f;
		L[i] = (float)((int32_t)lcg (seed) >> 8) * (1.0f / 8388608.0f) * s;
		R[i] = (float)((int32_t)lcg (seed) >> 8) * (1.0f / 8388608.0f) * s;
	}

	/* one call */
	std::unique_ptr<float[]>         hl (new float[Hn]), hr (new float[Hn]), oL (new float[n]), oR (new float[n]);
	std::unique_ptr<tbf_limit_meter> m (new tbf_limit_meter);
	memset (hl.get (), 0, Hn * sizeof (float)), memset (hr.get (), 0, Hn * sizeof (float));
	CHECK (tbf_debug_limit_tp_ref (&cfg, &det, L.get (), R.get (), n, hl.get (), hr.get (), oL.get (), oR.get (), m.get ()) == 0);
	CHECK (m->reduced > 0u && m->min_gain < 1.0f && m->min_gain > 0.0f);
	for (uint32_t i = 0; i < n; i++)
		CHECK (fabsf (oL[i]) <= cfg.ceiling && fabsf (oR[i]) <= cfg.ceiling);
	if (n >= Hn)
		CHECK (memcmp (hl.get (), L.get () + n - Hn, Hn * sizeof (float)) == 0 && memcmp (hr.get (), R.get () + n - Hn, Hn * sizeof (float)) == 0);

	/* the cuts: single ones and all of them together */
	const std::vector<uint32_t>        sizes = {1u, 5u, 6u, 7u, 11u, 12u, D + 6u, Hn + 3u};
	std::vector<std::vector<uint32_t>> cuts;
	std::vector<uint32_t>              all;
	uint32_t                           at = 0;
	for (uint32_t s : sizes) {
		if (s < n)
			cuts.push_back ({s});
		if (at + s < n)
			all.push_back (at += s);
	}
	cuts.push_back (all);
	for (const auto& cut : cuts) {
		std::unique_ptr<float[]> cl (new float[Hn]), cr (new float[Hn]);
		memset (cl.get (), 0, Hn * sizeof (float)), memset (cr.get (), 0, Hn * sizeof (float));
		std::vector<uint32_t> edge = {0u};
		edge.insert (edge.end (), cut.begin (), cut.end ());
		edge.push_back (n);
		std::vector<float> joined[2];
		uint32_t           reduced = 0, clamped = 0;
		float              minG = 1.0f;
		for (size_t k = 0; k + 1 < edge.size (); k++) {
			const uint32_t a = edge[k], len = edge[k + 1] - a;
			/* the segment as heap arrays of its own, so that its ends are guarded */
			std::unique_ptr<float[]> l (new float[len]), r (new float[len]), yl (new float[len]), yr (new float[len]);
			std::unique_ptr<tbf_limit_meter> cm (new tbf_limit_meter);
			memcpy (l.get (), L.get () + a, len * sizeof (float));
			memcpy (r.get (), R.get () + a, len * sizeof (float));
			CHECK (tbf_debug_limit_tp_ref (&cfg, &det, l.get (), r.get (), len, cl.get (), cr.get (), yl.get (), yr.get (), cm.get ()) == 0);
			joined[0].insert (joined[0].end (), yl.get (), yl.get () + len);
			joined[1].insert (joined[1].end (), yr.get (), yr.get () + len);
			reduced += cm->reduced, clamped += cm->clamped, minG = std::min (minG, cm->min_gain);
		}
		CHECK (joined[0].size () == n && memcmp (joined[0].data (), oL.get (), n * sizeof (float)) == 0);
		CHECK (joined[1].size () == n && memcmp (joined[1].data (), oR.get (), n * sizeof (float)) == 0);
		CHECK (memcmp (cl.get (), hl.get (), Hn * sizeof (float)) == 0 && memcmp (cr.get (), hr.get (), Hn * sizeof (float)) == 0);
		CHECK (reduced == m->reduced && clamped == m->clamped && minG == m->min_gain);
	}
	/* no frames: nothing moves, the planes may be NULL, and so may the meter */
	CHECK (tbf_debug_limit_tp_ref (&cfg, &det, nullptr, nullptr, 0, hl.get (), hr.get (), nullptr, nullptr, nullptr) == 0);
	/* mono: one plane passed twice */
	CHECK (tbf_debug_limit_tp_ref (&cfg, &det, L.get (), L.get (), n, hl.get (), hr.get (), oL.get (), oR.get (), nullptr) == 0);
	printf ("limit_tp_san: A = %u, H = %u, F = %u, %u frames: one call and %zu cuts agree, %u frames reduced, least gain %.4f\n", A, H, F,
	        n, cuts.size (), m->reduced, m->min_gain);
	return 0;
}

static int refusals ()
{
	tbf_engine_config ec;
	memset (&ec, 0, sizeof (ec));
	ec.sample_rate = 48000.0;
	ec.device      = -1;
	tbf_engine* e = nullptr;
	CHECK (tbf_engine_create (&ec, &e) == 0 && e);
	tbf_limiter*       lim = nullptr;
	tbf_limiter_config cfg = {0.5f, 64u, 1u};
	tbf_limiter_detect det = {4u, 0u};
	CHECK (tbf_limiter_create_tp (e, 4u, &cfg, &det, &lim) == -19 && !lim);
	det.oversample = 3u;
	CHECK (tbf_limiter_create_tp (e, 4u, &cfg, &det, &lim) == -22);
	det = {2u, 1u};
	CHECK (tbf_limiter_create_tp (e, 4u, &cfg, &det, &lim) == -22);
	CHECK (tbf_limiter_create_tp (e, 4u, &cfg, nullptr, &lim) == -22);
	det = {2u, 0u};
	cfg.ahead = 48u;
	CHECK (tbf_limiter_create_tp (e, 4u, &cfg, &det, &lim) == -22);
	CHECK (tbf_debug_limit_tp_grid (&cfg, &det, nullptr, nullptr, nullptr, nullptr) == -22);
	CHECK (tbf_engine_destroy (e) == 0);
	printf ("limit_tp_san: a host-only engine validates, then refuses\n");
	return 0;
}

int main ()
{
	if (run (2u, 0u, 4u, 700u) || run (64u, 1u, 4u, 700u) || run (64u, 1u, 2u, 701u) || run (16u, 5u, 4u, 333u) || run (512u, 4096u, 2u, 6000u) ||
	    run (64u, 200u, 4u, 40u) || refusals ())
		return 1;
	printf ("limit_tp_san: ok\n");
	return 0;
}
