/*
 * tools/loudness_san.cpp -- the loudness meter's host code under AddressSanitizer + UBSan
 * (make -C tunebfree_amd loudness_san; a CPU program, no device): tbf_debug_loudness_coeffs,
 * tbf_debug_loudness_ref and tbf_debug_loudness_result over heap arrays of exactly the sizes the
 * calls are entitled to, so that one element read or written beyond them is reported.  A row of
 * noise is taken in one call and in cuts at 1, Hp - 1, Hp, Hp + 1 and inside the third hop, at two
 * rates; both must give the same bits.  Exit code 0 and "loudness_san: ok" when everything held.
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
			fprintf (stderr, "loudness_san: %s failed (line %d): %s\n", #x, __LINE__, tbf_last_error ()); \
			return 1;                                                             \
		}                                                                         \
	} while (0)

static int run (uint32_t rate, uint32_t n)
{
	const uint32_t            Hp = rate / 10u, hops = n / Hp;
	const tbf_loudness_config cfg = {rate, 1u};
	std::unique_ptr<float[]>  L (new float[n]), R (new float[n]);
	uint32_t                  seed = rate;
	for (uint32_t i = 0; i < n; i++) {
		L[i] = (float)((int32_t)lcg (seed) >> 8) * (1.0f / 8388608.0f) * 0.25f;
		R[i] = (float)((int32_t)lcg (seed) >> 8) * (1.0f / 8388608.0f) * 0.25f;
	}
	std::unique_ptr<double[]> c (new double[7]);
	CHECK (tbf_debug_loudness_coeffs (rate, c.get ()) == 0);

	/* one call */
	std::unique_ptr<double[]> st (new double[12]), e (new double[2u * hops]);
	memset (st.get (), 0, 12 * sizeof (double));
	uint32_t got = 0;
	CHECK (tbf_debug_loudness_ref (&cfg, L.get (), R.get (), n, st.get (), e.get (), hops, &got) == 0 && got == hops);
	/* one hop too few: refused, nothing written */
	if (hops) {
		std::unique_ptr<double[]> st2 (new double[12]), e2 (new double[2u * (hops - 1u)]);
		memset (st2.get (), 0, 12 * sizeof (double));
		CHECK (tbf_debug_loudness_ref (&cfg, L.get (), R.get (), n, st2.get (), hops > 1u ? e2.get () : nullptr, hops - 1u, &got) == -28);
	}

	/* the cuts */
	const uint32_t            at[] = {0u, 1u, Hp - 1u, Hp, Hp + 1u, 2u * Hp + 37u, n};
	std::unique_ptr<double[]> cs (new double[12]);
	memset (cs.get (), 0, 12 * sizeof (double));
	std::vector<double> joined;
	for (int k = 0; k < 6; k++) {
		const uint32_t a = at[k], b = at[k + 1], len = b - a;
		const uint32_t need = ((uint32_t)cs[5] + len) / Hp;
		/* the segment as a heap array of its own, so that its ends are guarded */
		std::unique_ptr<float[]>  l (new float[len]), r (new float[len]);
		std::unique_ptr<double[]> ee (new double[2u * need]);
		memcpy (l.get (), L.get () + a, len * sizeof (float));
		memcpy (r.get (), R.get () + a, len * sizeof (float));
		CHECK (tbf_debug_loudness_ref (&cfg, l.get (), r.get (), len, cs.get (), ee.get (), need, &got) == 0 && got == need);
		joined.insert (joined.end (), ee.get (), ee.get () + 2u * need);
	}
	CHECK (joined.size () == 2u * hops && memcmp (joined.data (), e.get (), joined.size () * sizeof (double)) == 0);
	CHECK (memcmp (cs.get (), st.get (), 12 * sizeof (double)) == 0);

	/* the gating, on every prefix of the energies */
	for (uint32_t h = 0; h <= hops; h++) {
		std::unique_ptr<double[]>            p (new double[2u * h]);
		std::unique_ptr<tbf_loudness_result> res (new tbf_loudness_result);
		memcpy (p.get (), e.get (), 2u * h * sizeof (double));
		CHECK (tbf_debug_loudness_result (rate, h ? p.get () : nullptr, h, res.get ()) == 0);
		CHECK (res->hops == h && res->blocks == (h >= 4u ? h - 3u : 0u) && res->gated <= res->blocks);
		CHECK ((h >= 4u) == (res->momentary_max > -HUGE_VAL) && (h >= 30u) == (res->short_term_max > -HUGE_VAL));
	}
	printf ("loudness_san: rate %u, %u frames, %u hops: one call and the cuts agree\n", rate, n, hops);
	return 0;
}

int main ()
{
	if (run (8000u, 6000u) || run (8000u, 32u * 800u + 5u) || run (44100u, 3u * 4410u + 100u))
		return 1;
	printf ("loudness_san: ok\n");
	return 0;
}
