/*
 * tools/eq_san.cpp -- the bus equaliser's host code under AddressSanitizer + UBSan
 * (make -C tunebfree_amd eq_san; a CPU program, no device): tbf_debug_eq_coeffs over the nine types
 * at the corners of the accepted ranges and one step beyond each, tbf_debug_eq_ref over heap arrays
 * of exactly the sizes the calls are entitled to, so that one element read or written beyond them
 * is reported, and the argument checks of tbf_eq_create on a host-only engine.  A row of noise is
 * taken in one call and in cuts at 1, 7, 128, 129 and inside, with 0, 1, 3 and 8 bands; both must
 * give the same bits.  Exit code 0 and "eq_san: ok" when everything held.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

#include "tbf.h"

static uint32_t lcg (uint32_t& s) { return s = s * 1664525u + 1013904223u; }

#define CHECK(x)                                                                                        \
	do {                                                                                                \
		if (!(x)) {                                                                                     \
			fprintf (stderr, "eq_san: %s failed (line %d): %s\n", #x, __LINE__, tbf_last_error ()); \
			return 1;                                                                                   \
		}                                                                                               \
	} while (0)

static int designer ()
{
	const uint32_t rates[] = {8000u, 44100u, 48000u, 192000u};
	unsigned       n = 0;
	for (uint32_t rate : rates)
		for (int type = 0; type <= 8; type++) {
			const double hz[] = {0.0002 * rate * (1 + 1e-9) + 1e-9, 0.25 * rate, 0.4998 * rate * (1 - 1e-9)};
			const double q[]  = {0.1 + 1e-9, 0.7071, 6.0 - 1e-9};
			const double g[]  = {-24.0, 0.0, 24.0};
			for (double h : hz)
				for (double qq : q)
					for (double gg : g) {
						std::unique_ptr<tbf_eq_band> b (new tbf_eq_band{type, 0, h, qq, gg});
						std::unique_ptr<double[]>    c (new double[5]);
						CHECK (tbf_debug_eq_coeffs (rate, b.get (), c.get ()) == 0);
						for (int i = 0; i < 5; i++)
							CHECK (isfinite (c[i]));
						n++;
					}
			std::unique_ptr<double[]> c (new double[5]);
			const tbf_eq_band         bad[] = {{type, 0, 0.0002 * rate, 1.0, 0.0}, {type, 0, 0.4998 * rate, 1.0, 0.0}, {type, 0, 1000.0, 0.1, 0.0},
			                                   {type, 0, 1000.0, 6.0, 0.0},        {type, 0, 1000.0, 1.0, 24.5},       {type, 0, 1000.0, 1.0, NAN},
			                                   {type, 0, NAN, 1.0, 0.0},           {type, 0, 1000.0, NAN, 0.0}};
			for (const tbf_eq_band& b : bad)
				CHECK (tbf_debug_eq_coeffs (rate, &b, c.get ()) == -22 && strstr (tbf_last_error (), "row 0 band 0"));
		}
	const tbf_eq_band ok = {TBF_EQ_PEQ, 0, 1000.0, 1.0, 3.0}, t9 = {9, 0, 1000.0, 1.0, 3.0}, tm = {-1, 0, 1000.0, 1.0, 3.0};
	double            c5[5];
	CHECK (tbf_debug_eq_coeffs (7999u, &ok, c5) == -22 && tbf_debug_eq_coeffs (192001u, &ok, c5) == -22);
	CHECK (tbf_debug_eq_coeffs (48000u, &t9, c5) == -22 && tbf_debug_eq_coeffs (48000u, &tm, c5) == -22);
	CHECK (tbf_debug_eq_coeffs (48000u, nullptr, c5) == -22 && tbf_debug_eq_coeffs (48000u, &ok, nullptr) == -22);
	printf ("eq_san: %u bands designed at the corners, the steps beyond refused\n", n);
	return 0;
}

static int run (uint32_t nb, uint32_t n)
{
	const uint32_t rate = 8000u;
	std::unique_ptr<float[]> L (new float[n]), R (new float[n]);
	uint32_t                 seed = 77u + nb;
	for (uint32_t i = 0; i < n; i++) {
		L[i] = (float)((int32_t)lcg (seed) >> 8) * (1.0f / 8388608.0f) * 0.25f;
		R[i] = (float)((int32_t)lcg (seed) >> 8) * (1.0f / 8388608.0f) * 0.25f;
	}
	std::unique_ptr<double[]> c (new double[5u * nb]);
	for (uint32_t b = 0; b < nb; b++) {
		const tbf_eq_band bd = {(int32_t)((b + nb) % 9u), 0, 100.0 + 400.0 * b, 0.5 + 0.25 * b, -6.0 + 1.5 * b};
		CHECK (tbf_debug_eq_coeffs (rate, &bd, c.get () + 5u * b) == 0);
	}
	/* one call */
	std::unique_ptr<double[]> st (new double[4u * nb]);
	std::unique_ptr<float[]>  oL (new float[n]), oR (new float[n]);
	memset (st.get (), 0, 4u * nb * sizeof (double));
	CHECK (tbf_debug_eq_ref (nb ? c.get () : nullptr, nb, L.get (), R.get (), n, nb ? st.get () : nullptr, oL.get (), oR.get ()) == 0);
	/* the cuts */
	uint32_t                  at[] = {0u, 1u, 8u, 136u, 265u, n / 2u + 3u, n};
	for (uint32_t& v : at)
		v = v < n ? v : n; /* a short row: empty segments behind its end */
	std::unique_ptr<double[]> cs (new double[4u * nb]);
	memset (cs.get (), 0, 4u * nb * sizeof (double));
	std::vector<float> jl, jr;
	for (int k = 0; k < 6; k++) {
		const uint32_t a = at[k], len = at[k + 1] - a;
		/* the segment as heap arrays of its own, so that their ends are guarded */
		std::unique_ptr<float[]> l (new float[len]), r (new float[len]), ol (new float[len]), orr (new float[len]);
		memcpy (l.get (), L.get () + a, len * sizeof (float));
		memcpy (r.get (), R.get () + a, len * sizeof (float));
		CHECK (tbf_debug_eq_ref (nb ? c.get () : nullptr, nb, l.get (), r.get (), len, nb ? cs.get () : nullptr, ol.get (), orr.get ()) == 0);
		jl.insert (jl.end (), ol.get (), ol.get () + len);
		jr.insert (jr.end (), orr.get (), orr.get () + len);
	}
	CHECK (jl.size () == n && memcmp (jl.data (), oL.get (), n * sizeof (float)) == 0 && memcmp (jr.data (), oR.get (), n * sizeof (float)) == 0);
	CHECK (memcmp (cs.get (), st.get (), 4u * nb * sizeof (double)) == 0);
	if (nb == 0)
		CHECK (memcmp (oL.get (), L.get (), n * sizeof (float)) == 0 && memcmp (oR.get (), R.get (), n * sizeof (float)) == 0);
	/* one plane as both channels */
	std::unique_ptr<double[]> ms (new double[4u * nb]);
	std::unique_ptr<float[]>  mL (new float[n]), mR (new float[n]);
	memset (ms.get (), 0, 4u * nb * sizeof (double));
	CHECK (tbf_debug_eq_ref (nb ? c.get () : nullptr, nb, L.get (), L.get (), n, nb ? ms.get () : nullptr, mL.get (), mR.get ()) == 0);
	CHECK (memcmp (mL.get (), oL.get (), n * sizeof (float)) == 0 && memcmp (mR.get (), oL.get (), n * sizeof (float)) == 0);
	printf ("eq_san: %u bands, %u frames: one call and the cuts agree\n", nb, n);
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
	tbf_eq*             eq  = nullptr;
	const tbf_eq_config ok = {48000u, 8u}, r0 = {7999u, 8u}, r1 = {192001u, 8u}, b0 = {48000u, 0u}, b9 = {48000u, 9u};
	CHECK (tbf_eq_create (e, 4u, &ok, &eq) == -19 && eq == nullptr);
	CHECK (tbf_eq_create (nullptr, 4u, &ok, &eq) == -22 && tbf_eq_create (e, 4u, &ok, nullptr) == -22);
	CHECK (tbf_eq_create (e, 4u, nullptr, &eq) == -22 && tbf_eq_create (e, 0u, &ok, &eq) == -22);
	CHECK (tbf_eq_create (e, 4u, &r0, &eq) == -22 && tbf_eq_create (e, 4u, &r1, &eq) == -22);
	CHECK (tbf_eq_create (e, 4u, &b0, &eq) == -22 && tbf_eq_create (e, 4u, &b9, &eq) == -22);
	uint32_t nb = 0;
	CHECK (tbf_eq_destroy (nullptr) == 0 && tbf_eq_reset (nullptr, 0u, nullptr, nullptr) == -22);
	CHECK (tbf_eq_set (nullptr, 0u, nullptr, nullptr, nullptr, nullptr) == -22 && tbf_eq_bands (nullptr, 0u, nullptr, 0u, &nb) == -22);
	CHECK (tbf_eq_device (nullptr, nullptr, nullptr, 0u, 0u, nullptr, nullptr, 0u, nullptr, nullptr) == -22);
	uint32_t P = 0, rows = 0, tile = 0, lds = 0;
	for (uint32_t mb = 1; mb <= 8u; mb++)
		CHECK (tbf_debug_eq_grid (mb, &P, &rows, &tile, &lds) == 0 && P >= mb && P < 2u * mb && P * rows == 32u && lds <= 160u * 1024u);
	CHECK (tbf_debug_eq_grid (0u, &P, &rows, &tile, &lds) == -22 && tbf_debug_eq_grid (9u, nullptr, nullptr, nullptr, nullptr) == -22);
	CHECK (tbf_engine_destroy (e) == 0);
	printf ("eq_san: a host-only engine's equaliser: validated, then -19\n");
	return 0;
}

int main ()
{
	if (designer () || run (0u, 3000u) || run (1u, 3000u) || run (3u, 3000u) || run (8u, 3000u) || run (8u, 1u) || hostOnly ())
		return 1;
	printf ("eq_san: ok\n");
	return 0;
}
