/*
 * tools/comp_san.cpp -- the bus compressor's host code under AddressSanitizer + UBSan
 * (make -C tunebfree_amd comp_san; a CPU program, no device): tbf_comp_curve_design at the corners
 * of the accepted ranges and one step beyond each, tbf_debug_comp_lookup and tbf_debug_comp_ref over
 * heap arrays of exactly the sizes the calls are entitled to, so that one element read or written
 * beyond them is reported, and the argument checks of tbf_comp_create on a host-only engine.  The
 * lookup takes every grid level, both ends of the grid, zero, denormals and +Inf; a row whose level
 * wanders over 30 octaves, with NaN and Inf in it, is taken in one call and in cuts at 1, 3, 127 and
 * inside, with and without a key; both must give the same bits.  Exit code 0 and "comp_san: ok"
 * when everything held.
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

#define CHECK(x)                                                                                          \
	do {                                                                                                  \
		if (!(x)) {                                                                                       \
			fprintf (stderr, "comp_san: %s failed (line %d): %s\n", #x, __LINE__, tbf_last_error ()); \
			return 1;                                                                                     \
		}                                                                                                 \
	} while (0)

static int designer ()
{
	const double T[] = {-90.0, -20.0, 0.0}, R[] = {1.0, 4.0, INFINITY}, W[] = {0.0, 6.0, 40.0};
	unsigned     n = 0;
	for (double t : T)
		for (double r : R)
			for (double w : W) {
				std::unique_ptr<float[]> p (new float[TBF_COMP_POINTS]);
				CHECK (tbf_comp_curve_design (t, r, w, p.get ()) == 0);
				for (uint32_t i = 0; i < TBF_COMP_POINTS; i++)
					CHECK (p[i] > 0.0f && p[i] <= 1.0f && (i == 0 || p[i] <= p[i - 1]) && (r != 1.0 || p[i] == 1.0f));
				n++;
			}
	std::unique_ptr<float[]> p (new float[TBF_COMP_POINTS]);
	const double             bad[][3] = {{-90.5, 4, 0}, {0.5, 4, 0}, {NAN, 4, 0}, {-20, 0.5, 0}, {-20, NAN, 0}, {-20, 4, -1}, {-20, 4, 41}, {-20, 4, NAN}};
	for (const auto& b : bad)
		CHECK (tbf_comp_curve_design (b[0], b[1], b[2], p.get ()) == -22);
	CHECK (tbf_comp_curve_design (-20.0, 4.0, 0.0, nullptr) == -22);
	printf ("comp_san: %u curves designed at the corners, the steps beyond refused\n", n);
	return 0;
}

static int lookup ()
{
	std::unique_ptr<float[]> p (new float[TBF_COMP_POINTS]);
	CHECK (tbf_comp_curve_design (-30.0, 4.0, 6.0, p.get ()) == 0);
	std::unique_ptr<float[]> lv (new float[TBF_COMP_POINTS]), t (new float[TBF_COMP_POINTS]);
	for (uint32_t i = 0; i < TBF_COMP_POINTS; i++)
		lv[i] = ldexpf (1.0f + (float)(i % TBF_COMP_SEG) / (float)TBF_COMP_SEG, (int)(i / TBF_COMP_SEG) - 16);
	CHECK (tbf_debug_comp_lookup (p.get (), lv.get (), TBF_COMP_POINTS, t.get ()) == 0);
	CHECK (memcmp (t.get (), p.get (), TBF_COMP_POINTS * sizeof (float)) == 0);
	const float              edge[] = {0.0f, 1e-45f, 1e-38f, nextafterf (0x1p-16f, 0.0f), 0x1p-16f, 254.0f, 256.0f, 3e38f, INFINITY};
	const uint32_t           ne = sizeof (edge) / sizeof (edge[0]);
	std::unique_ptr<float[]> e (new float[ne]), te (new float[ne]);
	memcpy (e.get (), edge, sizeof (edge));
	CHECK (tbf_debug_comp_lookup (p.get (), e.get (), ne, te.get ()) == 0);
	for (uint32_t i = 0; i < ne; i++)
		CHECK (i == 5 ? te[i] > p[TBF_COMP_POINTS - 1u] && te[i] < p[TBF_COMP_POINTS - 2u] /* the middle of the last segment: not clamped */
		              : te[i] == (i < 5 ? p[0] : p[TBF_COMP_POINTS - 1u]));
	const float neg = -1.0f, nan = NAN;
	float       o;
	CHECK (tbf_debug_comp_lookup (p.get (), &neg, 1u, &o) == -22 && tbf_debug_comp_lookup (p.get (), &nan, 1u, &o) == -22);
	CHECK (tbf_debug_comp_lookup (nullptr, e.get (), ne, te.get ()) == -22 && tbf_debug_comp_lookup (p.get (), nullptr, 0u, nullptr) == 0);
	p[300] = 1.5f;
	CHECK (tbf_debug_comp_lookup (p.get (), e.get (), ne, te.get ()) == -22 && strstr (tbf_last_error (), "point 300"));
	printf ("comp_san: the lookup at every grid level, both clamps and the refusals\n");
	return 0;
}

static int run (uint32_t n, bool keyed, float a, float r, float m)
{
	std::unique_ptr<float[]> p (new float[TBF_COMP_POINTS]);
	CHECK (tbf_comp_curve_design (-35.0, keyed ? INFINITY : 3.0, 4.0, p.get ()) == 0);
	std::unique_ptr<float[]> L (new float[n]), R (new float[n]), kL (new float[n]), kR (new float[n]);
	uint32_t                 seed = 77u + n;
	for (uint32_t i = 0; i < n; i++) {
		float* const at[] = {&L[i], &R[i], &kL[i], &kR[i]};
		for (float* x : at)
			*x = ldexpf ((float)((int32_t)lcg (seed) >> 8) * (1.0f / 8388608.0f), (int)(lcg (seed) >> 27) - 21);
	}
	if (n > 40u) {
		L[7] = NAN, R[9] = INFINITY, kL[11] = NAN, kR[13] = -INFINITY, L[20] = -0.0f, R[21] = 1e-42f;
	}
	const float* const k0 = keyed ? kL.get () : nullptr;
	const float* const k1 = keyed ? kR.get () : nullptr;
	/* one call */
	float                    g = 1.0f;
	std::unique_ptr<float[]> oL (new float[n]), oR (new float[n]), og (new float[n]);
	CHECK (tbf_debug_comp_ref (p.get (), a, r, m, L.get (), R.get (), k0, k1, n, &g, oL.get (), oR.get (), og.get ()) == 0);
	for (uint32_t i = 0; i < n; i++)
		CHECK (og[i] >= 0.0f && og[i] <= 1.0f);
	/* the cuts */
	uint32_t at[] = {0u, 1u, 4u, 131u, 132u, n / 2u + 3u, n};
	for (uint32_t& v : at)
		v = v < n ? v : n; /* a short row: empty segments behind its end */
	std::sort (at, at + 7);
	float              cg = 1.0f;
	std::vector<float> jl, jr, jg;
	for (int k = 0; k < 6; k++) {
		const uint32_t b = at[k], len = at[k + 1] - b;
		/* the segment as heap arrays of its own, so that their ends are guarded */
		std::unique_ptr<float[]> l (new float[len]), rr (new float[len]), kl (new float[len]), kr (new float[len]), ol (new float[len]),
		    orr (new float[len]), gg (new float[len]);
		memcpy (l.get (), L.get () + b, len * sizeof (float));
		memcpy (rr.get (), R.get () + b, len * sizeof (float));
		memcpy (kl.get (), kL.get () + b, len * sizeof (float));
		memcpy (kr.get (), kR.get () + b, len * sizeof (float));
		CHECK (tbf_debug_comp_ref (p.get (), a, r, m, l.get (), rr.get (), keyed ? kl.get () : nullptr, keyed ? kr.get () : nullptr, len, &cg,
		                           ol.get (), orr.get (), gg.get ()) == 0);
		jg.insert (jg.end (), gg.get (), gg.get () + len);
		jl.insert (jl.end (), ol.get (), ol.get () + len);
		jr.insert (jr.end (), orr.get (), orr.get () + len);
	}
	CHECK (jl.size () == n && memcmp (jl.data (), oL.get (), n * sizeof (float)) == 0 && memcmp (jr.data (), oR.get (), n * sizeof (float)) == 0);
	CHECK (jg.size () == n && memcmp (jg.data (), og.get (), n * sizeof (float)) == 0 && memcmp (&cg, &g, sizeof (float)) == 0);
	/* one plane as both channels */
	float                    mg = 1.0f;
	std::unique_ptr<float[]> mL (new float[n]), mR (new float[n]);
	CHECK (tbf_debug_comp_ref (p.get (), a, r, m, L.get (), L.get (), k0, k1, n, &mg, mL.get (), mR.get (), nullptr) == 0);
	CHECK (memcmp (mL.get (), mR.get (), n * sizeof (float)) == 0);
	printf ("comp_san: %u frames%s: one call and the cuts agree\n", n, keyed ? ", keyed" : "");
	return 0;
}

static int flat ()
{
	const uint32_t           n = 500u;
	std::unique_ptr<float[]> p (new float[TBF_COMP_POINTS]), L (new float[n]), o (new float[n]), o2 (new float[n]);
	for (uint32_t i = 0; i < TBF_COMP_POINTS; i++)
		p[i] = 1.0f;
	uint32_t seed = 5u;
	for (uint32_t i = 0; i < n; i++)
		L[i] = ldexpf ((float)((int32_t)lcg (seed) >> 8) * (1.0f / 8388608.0f), (int)(lcg (seed) >> 26) - 40);
	float g = 1.0f;
	CHECK (tbf_debug_comp_ref (p.get (), 0.9f, 0.99f, 1.0f, L.get (), L.get (), nullptr, nullptr, n, &g, o.get (), o2.get (), nullptr) == 0);
	CHECK (g == 1.0f && memcmp (o.get (), L.get (), n * sizeof (float)) == 0 && memcmp (o2.get (), L.get (), n * sizeof (float)) == 0);
	/* the refusals of the restatement */
	const float bad[][3] = {{1.0f, 0.0f, 1.0f}, {-0.1f, 0.0f, 1.0f}, {NAN, 0.0f, 1.0f}, {0.0f, 1.0f, 1.0f}, {0.0f, NAN, 1.0f}, {0.0f, 0.0f, 256.5f},
	                        {0.0f, 0.0f, -1.0f}, {0.0f, 0.0f, NAN}, {0.0f, 0.0f, INFINITY}};
	for (const auto& b : bad)
		CHECK (tbf_debug_comp_ref (p.get (), b[0], b[1], b[2], L.get (), L.get (), nullptr, nullptr, n, &g, o.get (), o2.get (), nullptr) == -22 &&
		       strstr (tbf_last_error (), "row 0"));
	float gb = 1.5f;
	CHECK (tbf_debug_comp_ref (p.get (), 0.0f, 0.0f, 1.0f, L.get (), L.get (), nullptr, nullptr, n, &gb, o.get (), o2.get (), nullptr) == -22);
	CHECK (tbf_debug_comp_ref (p.get (), 0.0f, 0.0f, 1.0f, L.get (), L.get (), L.get (), nullptr, n, &g, o.get (), o2.get (), nullptr) == -22);
	CHECK (tbf_debug_comp_ref (p.get (), 0.0f, 0.0f, 1.0f, nullptr, nullptr, nullptr, nullptr, 0u, &g, nullptr, nullptr, nullptr) == 0);
	printf ("comp_san: a flat curve is the identity, the restatement's refusals\n");
	return 0;
}

static int hostOnly ()
{
	tbf_engine_config ec;
	memset (&ec, 0, sizeof (ec));
	ec.sample_rate = 48000.0;
	ec.device      = -1;
	tbf_engine* e  = nullptr;
	CHECK (tbf_engine_create (&ec, &e) == 0 && e);
	tbf_comp*             cp = nullptr;
	const tbf_comp_config ok = {8u}, c0 = {0u}, c9 = {9u};
	CHECK (tbf_comp_create (e, 4u, &ok, &cp) == -19 && cp == nullptr);
	CHECK (tbf_comp_create (nullptr, 4u, &ok, &cp) == -22 && tbf_comp_create (e, 4u, &ok, nullptr) == -22);
	CHECK (tbf_comp_create (e, 4u, nullptr, &cp) == -22 && tbf_comp_create (e, 0u, &ok, &cp) == -22);
	CHECK (tbf_comp_create (e, 4u, &c0, &cp) == -22 && tbf_comp_create (e, 4u, &c9, &cp) == -22);
	tbf_comp_row row;
	float        pt;
	CHECK (tbf_comp_destroy (nullptr) == 0 && tbf_comp_reset (nullptr, 0u, nullptr, nullptr) == -22);
	CHECK (tbf_comp_curve_set (nullptr, 0u, &pt, nullptr) == -22 && tbf_comp_rows_set (nullptr, 0u, nullptr, &row, nullptr) == -22);
	CHECK (tbf_comp_curve_get (nullptr, 0u, &pt) == -22 && tbf_comp_row_get (nullptr, 0u, &row) == -22);
	CHECK (tbf_comp_device (nullptr, nullptr, nullptr, 0u, 0u, nullptr, nullptr, 0u, nullptr, nullptr, 0u, nullptr, nullptr, nullptr) == -22);
	CHECK (tbf_debug_comp_time (nullptr, 0, nullptr, nullptr) == -22);
	uint32_t rows = 0, tile = 0, lds = 0;
	for (uint32_t n = 1; n <= (1u << 22); n *= 3u)
		for (uint32_t nc = 1; nc <= TBF_COMP_MAX_CURVES; nc++)
			CHECK (tbf_debug_comp_grid (n, nc, &rows, &tile, &lds) == 0 && rows >= 1u && rows <= 64u && tile >= 64u && lds <= 160u * 1024u);
	CHECK (tbf_debug_comp_grid (0u, 1u, &rows, &tile, &lds) == -22 && tbf_debug_comp_grid (4u, 0u, nullptr, nullptr, nullptr) == -22);
	CHECK (tbf_debug_comp_grid (4u, 9u, nullptr, nullptr, nullptr) == -22 && tbf_debug_comp_grid (4u, 1u, nullptr, nullptr, nullptr) == 0);
	CHECK (tbf_engine_destroy (e) == 0);
	printf ("comp_san: a host-only engine's compressor: validated, then -19\n");
	return 0;
}

int main ()
{
	if (designer () || lookup () || run (3000u, false, 0.9f, 0.999f, 2.0f) || run (3000u, true, 0.0f, 0.5f, 1.0f) ||
	    run (1u, false, 0.5f, 0.5f, 1.0f) || run (130u, true, 0.99f, 0.0f, 0.5f) || flat () || hostOnly ())
		return 1;
	printf ("comp_san: ok\n");
	return 0;
}
