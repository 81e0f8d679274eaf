/*
 * tools/truepeak_san.cpp -- the true-peak meter's host code and the loudness range under
 * AddressSanitizer + UBSan (make -C tunebfree_amd truepeak_san; a CPU program, no device):
 * tbf_debug_true_peak_table, tbf_debug_true_peak_ref, tbf_debug_true_peak_dbtp and
 * tbf_debug_loudness_range over heap arrays of exactly the sizes the calls are entitled to, so that
 * one element read or written beyond them is reported.  A row of noise with an aimed burst is taken
 * in one call and in cuts at 1, 10, 11, 12 frames and at every frame from 11 before the burst to 1
 * behind it, at every oversampling factor; peaks and history must be the same bits, and the y of the
 * cuts joined must be the y of the one call.  The range runs on every prefix of a hop list.  Exit
 * code 0 and "truepeak_san: ok" when everything held.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "tbf.h"

static uint32_t lcg (uint32_t& s) { return s = s * 1664525u + 1013904223u; }

#define CHECK(x)                                                                  \
	do {                                                                          \
		if (!(x)) {                                                               \
			fprintf (stderr, "truepeak_san: %s failed (line %d): %s\n", #x, __LINE__, tbf_last_error ()); \
			return 1;                                                             \
		}                                                                         \
	} while (0)

static int run (uint32_t F, uint32_t n, uint32_t n0)
{
	const uint32_t             P = F == 1u ? 0u : F;
	const tbf_true_peak_config cfg = {F, 0u};
	std::unique_ptr<float[]>   h (new float[48]), L (new float[n]), R (new float[n]);
	CHECK (tbf_debug_true_peak_table (h.get ()) == 0);
	uint32_t seed = F * 977u + n;
	for (uint32_t i = 0; i < n; i++) {
		L[i] = (float)((int32_t)lcg (seed) >> 8) * (1.0f / 8388608.0f) * 0.01f;
		R[i] = (float)((int32_t)lcg (seed) >> 8) * (1.0f / 8388608.0f) * 0.01f;
	}
	for (uint32_t j = 0; j < 12u; j++) { /* the burst matched to phase 1 in L and to phase 3, 5 frames on, in R */
		L[n0 - j]      = h[12u + j] / h[12u + 6u];
		R[n0 + 5u - j] = h[36u + j] / h[36u + 5u];
	}

	/* one call */
	std::unique_ptr<float[]>    hist (new float[22]), y (new float[2u * n * P]);
	std::unique_ptr<uint32_t[]> pk (new uint32_t[4]);
	memset (hist.get (), 0, 22 * sizeof (float));
	memset (pk.get (), 0, 4 * sizeof (uint32_t));
	CHECK (tbf_debug_true_peak_ref (&cfg, L.get (), R.get (), n, hist.get (), pk.get (), P ? y.get () : nullptr) == 0);
	CHECK (memcmp (hist.get (), L.get () + n - 11u, 11 * sizeof (float)) == 0 && memcmp (hist.get () + 11, R.get () + n - 11u, 11 * sizeof (float)) == 0);
	if (F == 4u) { /* the maximum sits where it was aimed */
		uint32_t m;
		memcpy (&m, &y[(size_t)n0 * P + 1u], 4);
		CHECK ((m & 0x7fffffffu) == pk[2]);
		memcpy (&m, &y[((size_t)n + n0 + 5u) * P + 3u], 4);
		CHECK ((m & 0x7fffffffu) == pk[3]);
	}
	std::unique_ptr<double> db (new double);
	CHECK (tbf_debug_true_peak_dbtp (pk.get (), db.get ()) == 0 && *db > -0.1 && *db < 2.0);

	/* the cuts: single ones and all of them together */
	std::vector<std::vector<uint32_t>> cuts = {{1u}, {10u}, {11u}, {12u}, {1u, 10u, 11u, 12u, 23u}};
	for (uint32_t c = n0 - 11u; c <= n0 + 1u; c++)
		cuts.push_back ({c});
	for (const auto& cut : cuts) {
		std::unique_ptr<float[]>    ch (new float[22]);
		std::unique_ptr<uint32_t[]> cp (new uint32_t[4]);
		memset (ch.get (), 0, 22 * sizeof (float));
		memset (cp.get (), 0, 4 * sizeof (uint32_t));
		std::vector<uint32_t> at = {0u};
		at.insert (at.end (), cut.begin (), cut.end ());
		at.push_back (n);
		std::vector<float> joined[2];
		for (size_t k = 0; k + 1 < at.size (); k++) {
			const uint32_t a = at[k], len = at[k + 1] - a;
			/* the segment as heap arrays of its own, so that its ends are guarded */
			std::unique_ptr<float[]> l (new float[len]), r (new float[len]), yy (new float[2u * len * P]);
			memcpy (l.get (), L.get () + a, len * sizeof (float));
			memcpy (r.get (), R.get () + a, len * sizeof (float));
			CHECK (tbf_debug_true_peak_ref (&cfg, l.get (), r.get (), len, ch.get (), cp.get (), P ? yy.get () : nullptr) == 0);
			joined[0].insert (joined[0].end (), yy.get (), yy.get () + (size_t)len * P);
			joined[1].insert (joined[1].end (), yy.get () + (size_t)len * P, yy.get () + 2u * (size_t)len * P);
		}
		CHECK (memcmp (cp.get (), pk.get (), 4 * sizeof (uint32_t)) == 0);
		CHECK (memcmp (ch.get (), hist.get (), 22 * sizeof (float)) == 0);
		for (int c = 0; c < 2; c++)
			CHECK (joined[c].size () == (size_t)n * P && (P == 0u || memcmp (joined[c].data (), y.get () + (size_t)c * n * P, (size_t)n * P * sizeof (float)) == 0));
	}
	/* no frames: nothing moves, and the planes may be NULL */
	CHECK (tbf_debug_true_peak_ref (&cfg, nullptr, nullptr, 0, hist.get (), pk.get (), nullptr) == 0);
	printf ("truepeak_san: F = %u, %u frames, burst at %u: one call and %zu cuts agree, %.3f dBTP\n", F, n, n0, cuts.size (), *db);
	return 0;
}

static int range (uint32_t rate, uint32_t hops)
{
	std::unique_ptr<double[]> e (new double[2u * hops]);
	uint32_t                  seed = rate + hops;
	for (uint32_t h = 0; h < hops; h++) { /* levels between -80 and -10 dB, some hops silent */
		const double db = -80.0 + 70.0 * (double)(lcg (seed) >> 8) / 16777216.0;
		e[2u * h] = e[2u * h + 1u] = (h % 17u == 3u) ? 0.0 : (double)(rate / 10u) * pow (10.0, db / 10.0);
	}
	double last = 0.0;
	for (uint32_t h = 0; h <= hops; h++) {
		std::unique_ptr<double[]> p (new double[2u * h]);
		std::unique_ptr<double>   lra (new double);
		std::unique_ptr<uint32_t> win (new uint32_t);
		memcpy (p.get (), e.get (), 2u * h * sizeof (double));
		CHECK (tbf_debug_loudness_range (rate, h ? p.get () : nullptr, h, lra.get (), win.get ()) == 0);
		CHECK (*win <= (h >= 30u ? h - 29u : 0u) && *lra >= 0.0 && (*win > 0u || *lra == 0.0));
		CHECK (tbf_debug_loudness_range (rate, h ? p.get () : nullptr, h, lra.get (), nullptr) == 0);
		last = *lra;
	}
	printf ("truepeak_san: rate %u, every prefix of %u hops: range of all %.3f LU\n", rate, hops, last);
	return 0;
}

int main ()
{
	if (run (4u, 600u, 300u) || run (2u, 257u, 40u) || run (1u, 100u, 30u) || run (4u, 40u, 11u) || range (48000u, 200u) || range (8000u, 31u))
		return 1;
	printf ("truepeak_san: ok\n");
	return 0;
}
