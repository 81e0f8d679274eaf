/*
 * tools/remove_fuzz.cpp -- random add / clone / remove / step / save / load calls on a
 * host-only engine (device -1: the control plane alone), for an AddressSanitizer / UBSan build
 * of the host code.  Stand-alone: it has its own main, runs on the CPU and needs no GPU.
 *
 * Engine A takes every call.  Engine B, the shadow, never removes anything: every organ A ever
 * held has an instance there (twin[i] is A's instance i in B), and every note, parameter,
 * programme install, retune, step, clone and load A's instance gets, its twin gets too.
 * After each removal A's map is compared with the shadow list's, and every survivor's control
 * vector (tbf_debug_control) and next program (tbf_debug_render_program) with its twin's: an
 * array left uncompacted, or a removed instance's state left behind, shows as a difference,
 * an index past an array as a sanitizer report.  Both engines are rebuilt every few hundred
 * calls so that the shadow stays small.
 * Every few dozen calls the mixdown stage's host code runs too (mix): the host restatement
 * tbf_debug_mix_ref over random rows, buses and counts in heap arrays of the exact size, so that a
 * frame or a list entry past its end is a sanitizer report, and tbf_render_mix on A's instances,
 * which checks its rows and builds its list before it answers -19.
 *
 * Build and run: `make -C tunebfree_amd remove_fuzz` (the host sources compiled with
 * -fsanitize=address,undefined, linked with the kernels' objects as built), then
 * `tunebfree_amd/_build/remove_fuzz [calls [seed]]`.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <vector>

#include "../include/tbf.h"

#define CHECK(x)                                                                                   \
	do {                                                                                           \
		if (!(x)) {                                                                                \
			fprintf (stderr, "remove_fuzz: %s failed at line %d, call %d (%s)\n", #x, __LINE__, g_call, \
			         tbf_last_error ());                                                           \
			exit (1);                                                                              \
		}                                                                                          \
	} while (0)

static int g_call = 0;

struct Pair {
	tbf_engine*           a = nullptr;
	tbf_engine*           b = nullptr;
	uint32_t              tpl[2] = {0, 0};
	std::vector<uint32_t> twin; /* A's instance i is B's instance twin[i] */
};

static tbf_engine* organ (uint32_t tpl[2])
{
	tbf_engine_config cfg;
	memset (&cfg, 0, sizeof (cfg));
	cfg.sample_rate = 48000.0;
	cfg.device      = -1;
	tbf_engine* e   = nullptr;
	CHECK (tbf_engine_create (&cfg, &e) == 0 && e);
	CHECK (tbf_template_create (e, nullptr, nullptr, 7, &tpl[0]) == 0);
	CHECK (tbf_template_create (e, nullptr, nullptr, 8, &tpl[1]) == 0);
	CHECK (tbf_program_parse (e, "5 { name=\"any bars\", drawbars=random }\n") >= 0);
	return e;
}

static void compare (Pair& p, uint32_t i)
{
	double ca[64], cb[64];
	memset (ca, 0, sizeof (ca));
	memset (cb, 0, sizeof (cb));
	const int na = tbf_debug_control (p.a, i, ca, 64), nb = tbf_debug_control (p.b, p.twin[i], cb, 64);
	CHECK (na > 0 && na == nb && memcmp (ca, cb, sizeof (ca)) == 0);
}

/* one control step of A's instance i and its twin: the programs must be equal */
static void step (Pair& p, uint32_t i)
{
	static std::vector<float> pa (9 * 700), pb (9 * 700);
	const int na = tbf_debug_render_program (p.a, i, pa.data (), 700);
	const int nb = tbf_debug_render_program (p.b, p.twin[i], pb.data (), 700);
	CHECK (na >= 0 && na == nb && na <= 700);
	CHECK (memcmp (pa.data (), pb.data (), (size_t)na * 9 * sizeof (float)) == 0);
}

/* the mixdown stage's host code over exact-sized arrays; every sample against a plain loop */
static void mix (tbf_engine* e, std::mt19937& rng)
{
	auto           pick = [&] (uint32_t n) { return (uint32_t)(rng () % n); };
	const uint32_t n = pick (12), nb = pick (5), frames = 1 + pick (40), stride = frames + pick (3);
	const size_t   len = n ? (size_t)(n - 1) * stride + frames : 0; /* to the last row's last frame, no further */
	std::vector<float>       L (len), R (len);
	std::vector<uint32_t>    cnt (n);
	std::vector<tbf_mix_row> rows (n);
	for (float& v : L)
		v = (float)pick (2001) * 1e-3f - 1.0f;
	for (float& v : R)
		v = (float)pick (2001) * 1e-3f - 1.0f;
	for (uint32_t r = 0; r < n; r++) {
		rows[r] = {nb && pick (4) ? pick (nb) : TBF_MIX_NONE, (float)pick (5) * 0.5f - 1.0f, (float)pick (3) * 0.25f,
		           -(float)pick (3) * 0.25f, (float)pick (5) * 0.5f - 1.0f};
		cnt[r]  = pick (frames + 1);
	}
	const uint32_t     ostride = frames + pick (2);
	std::vector<float> oL ((size_t)nb * ostride + 1, 9.0f), oR ((size_t)nb * ostride + 1, 9.0f);
	const tbf_mix_out  out = {oL.data (), oR.data (), ostride};
	const bool         full = pick (3) == 0;
	CHECK (tbf_debug_mix_ref (n, L.data (), R.data (), stride, frames, full ? nullptr : cnt.data (), rows.data (), nb, &out) == 0);
	for (uint32_t b = 0; b < nb; b++)
		for (uint32_t j = 0; j < ostride; j++) {
			float al = 0.0f, ar = 0.0f;
			for (uint32_t r = 0; r < n && j < frames; r++)
				if (rows[r].bus == b && j < (full ? frames : cnt[r])) {
					const float xl = L[(size_t)r * stride + j], xr = R[(size_t)r * stride + j];
					al = __builtin_fmaf (rows[r].lr, xr, __builtin_fmaf (rows[r].ll, xl, al));
					ar = __builtin_fmaf (rows[r].rr, xr, __builtin_fmaf (rows[r].rl, xl, ar));
				}
			const float wl = j < frames ? al : 9.0f, wr = j < frames ? ar : 9.0f;
			CHECK (memcmp (&oL[(size_t)b * ostride + j], &wl, 4) == 0 && memcmp (&oR[(size_t)b * ostride + j], &wr, 4) == 0);
		}
	CHECK (oL.back () == 9.0f && oR.back () == 9.0f);
	/* on the engine's instances: the rows' checks and the list, then -19 (a host-only engine) */
	const uint32_t           ni = tbf_instance_count (e), buses = 1 + pick (3);
	std::vector<tbf_mix_row> ir (ni);
	for (uint32_t r = 0; r < ni; r++)
		ir[r] = {pick (3) ? pick (buses) : TBF_MIX_NONE, 1.0f, 0.0f, 0.0f, 1.0f};
	std::vector<float> hl ((size_t)buses * 128), hr ((size_t)buses * 128);
	const tbf_mix_out  ho = {hl.data (), hr.data (), 128};
	CHECK (tbf_render_mix (e, 1, ir.data (), buses, &ho) == -19);
	if (ni) {
		ir[pick (ni)].bus = buses;
		CHECK (tbf_render_mix (e, 1, ir.data (), buses, &ho) == -22);
	}
}

int main (int argc, char** argv)
{
	const int      calls = argc > 1 ? atoi (argv[1]) : 4000;
	const uint32_t seed  = argc > 2 ? (uint32_t)strtoul (argv[2], nullptr, 0) : 20241020u;
	std::mt19937   rng (seed);
	auto           pick = [&] (uint32_t n) { return (uint32_t)(rng () % n); };
	Pair           p;
	uint32_t       nextSeed = 1000, removals = 0, removed = 0, loads = 0, clones = 0;
	struct Blob {
		std::vector<unsigned char> bytes;
		uint32_t                   count;
	};
	std::vector<Blob> blobs;
	for (g_call = 0; g_call < calls; g_call++) {
		if (g_call % 400 == 0) { /* fresh engines: the shadow stays small */
			if (p.a)
				CHECK (tbf_engine_destroy (p.a) == 0 && tbf_engine_destroy (p.b) == 0);
			p.a = organ (p.tpl);
			p.b = organ (p.tpl);
			p.twin.clear ();
			blobs.clear ();
		}
		if (g_call % 37 == 0)
			mix (p.a, rng);
		const uint32_t n  = tbf_instance_count (p.a);
		uint32_t       op = pick (100);
		CHECK (n == p.twin.size ());
		if (n == 0 || (n < 3 && op < 40))
			op = 0;
		else if (n > 24)
			op = 50;
		if (op < 8) { /* add 1 .. 3 */
			const uint32_t k = 1 + pick (3);
			uint32_t       tp[3], sd[3], fa = 0, fb = 0;
			for (uint32_t q = 0; q < k; q++) {
				tp[q] = p.tpl[pick (2)];
				sd[q] = nextSeed++;
			}
			CHECK (tbf_instances_add (p.a, k, tp, sd, &fa) == 0 && fa == n);
			CHECK (tbf_instances_add (p.b, k, tp, sd, &fb) == 0);
			for (uint32_t q = 0; q < k; q++)
				p.twin.push_back (fb + q);
		} else if (op < 16) { /* clone 1 .. 3, repeats allowed */
			const uint32_t k = 1 + pick (3);
			uint32_t       sa[3], sb[3], fa = 0, fb = 0;
			for (uint32_t q = 0; q < k; q++) {
				sa[q] = pick (n);
				sb[q] = p.twin[sa[q]];
			}
			CHECK (tbf_instances_clone (p.a, k, sa, &fa) == 0 && fa == n);
			CHECK (tbf_instances_clone (p.b, k, sb, &fb) == 0);
			for (uint32_t q = 0; q < k; q++)
				p.twin.push_back (fb + q);
			clones += k;
		} else if (op < 30) { /* events: notes, parameters, a programme, a retune */
			const uint32_t i = pick (n), t = p.twin[i];
			for (uint32_t q = 0, m = 1 + pick (6); q < m; q++) {
				const uint32_t kind = pick (20);
				if (kind < 10) {
					const int32_t key = 36 + (int32_t)pick (60), on = (int32_t)pick (2);
					CHECK (tbf_note (p.a, i, key, on) == 0 && tbf_note (p.b, t, key, on) == 0);
				} else if (kind < 17) {
					const int32_t id = (int32_t)pick (20);
					const double  v  = id < 9 ? pick (9) : id < 13 ? pick (3) : pick (100) / 100.0;
					CHECK (tbf_set_param (p.a, i, id, v) == tbf_set_param (p.b, t, id, v));
				} else if (kind < 19) {
					CHECK (tbf_program_install (p.a, i, 4) == 0 && tbf_program_install (p.b, t, 4) == 0);
				} else {
					const uint32_t tp = p.tpl[pick (2)];
					CHECK (tbf_instance_retune (p.a, i, tp) == 0 && tbf_instance_retune (p.b, t, tp) == 0);
				}
			}
		} else if (op < 50) { /* step some */
			for (uint32_t q = 0, m = 1 + pick (n); q < m; q++)
				step (p, pick (n));
		} else if (op < 70) { /* remove: a random subset, sometimes all, sometimes a refused list */
			std::vector<uint32_t> all (n), map (n + 1, 12345u);
			for (uint32_t i = 0; i < n; i++)
				all[i] = i;
			std::shuffle (all.begin (), all.end (), rng);
			const uint32_t mode = pick (12);
			uint32_t       k    = mode == 0 ? n : mode == 1 ? 0 : 1 + pick (std::max (1u, n / 2));
			k                   = std::min (k, n);
			std::vector<uint32_t> gone (all.begin (), all.begin () + k);
			if (mode == 2 && k) { /* refused: a duplicate or an index past the end; nothing changes */
				gone.push_back (pick (2) ? gone[0] : n + pick (3));
				CHECK (tbf_instances_remove (p.a, (uint32_t)gone.size (), gone.data (), map.data ()) == -22);
				CHECK (tbf_instance_count (p.a) == n && map[0] == 12345u);
				for (uint32_t i = 0; i < n; i++)
					compare (p, i);
				continue;
			}
			CHECK (tbf_instances_remove (p.a, k, k ? gone.data () : nullptr, pick (4) ? map.data () : nullptr) == 0);
			CHECK (tbf_instance_count (p.a) == n - k);
			std::vector<uint8_t> dead (n, 0);
			for (uint32_t g : gone)
				dead[g] = 1;
			std::vector<uint32_t> tw;
			for (uint32_t i = 0; i < n; i++) {
				if (map[n] == 12345u && map[0] != 12345u) /* a map was asked for: it is the shadow's */
					CHECK (map[i] == (dead[i] ? UINT32_MAX : (uint32_t)tw.size ()));
				if (!dead[i])
					tw.push_back (p.twin[i]);
			}
			CHECK (map[n] == 12345u); /* nothing written past the old count */
			p.twin.swap (tw);
			for (uint32_t i = 0; i < n - k; i++)
				compare (p, i);
			for (uint32_t i = 0; i < n - k; i++)
				step (p, i);
			removals++;
			removed += k;
		} else if (op < 80) { /* save a few (from A; the twins' state is equal) */
			const uint32_t k = 1 + pick (std::min (n, 3u));
			uint32_t       inst[3];
			for (uint32_t q = 0; q < k; q++)
				inst[q] = pick (n);
			uint64_t size = 0;
			CHECK (tbf_instances_save (p.a, k, inst, nullptr, 0, &size) == 0 && size > 0);
			Blob bl;
			bl.bytes.resize (size);
			bl.count = k;
			CHECK (tbf_instances_save (p.a, k, inst, bl.bytes.data (), size, &size) == 0 && size == bl.bytes.size ());
			if (blobs.size () >= 6)
				blobs.erase (blobs.begin ());
			blobs.push_back (std::move (bl));
		} else if (op < 90 && !blobs.empty ()) { /* load one into distinct instances, and into their twins */
			const Blob& bl = blobs[pick ((uint32_t)blobs.size ())];
			if (bl.count > n)
				continue;
			std::vector<uint32_t> all (n);
			for (uint32_t i = 0; i < n; i++)
				all[i] = i;
			std::shuffle (all.begin (), all.end (), rng);
			uint32_t ia[3], ib[3];
			for (uint32_t q = 0; q < bl.count; q++) {
				ia[q] = all[q];
				ib[q] = p.twin[all[q]];
			}
			CHECK (tbf_instances_load (p.a, bl.count, ia, bl.bytes.data (), bl.bytes.size ()) == 0);
			CHECK (tbf_instances_load (p.b, bl.count, ib, bl.bytes.data (), bl.bytes.size ()) == 0);
			for (uint32_t q = 0; q < bl.count; q++)
				compare (p, ia[q]);
			loads++;
		} else { /* compare everything */
			for (uint32_t i = 0; i < n; i++)
				compare (p, i);
		}
	}
	uint64_t ib = 1, sb = 1;
	CHECK (tbf_debug_device_bytes (p.a, &ib, &sb) == 0 && ib == 0 && sb == 0);
	CHECK (tbf_engine_destroy (p.a) == 0 && tbf_engine_destroy (p.b) == 0);
	printf ("remove_fuzz: %d calls (seed %u): %u removals of %u instances, %u clones, %u loads, all survivors equal their shadows\n",
	        calls, seed, removals, removed, clones, loads);
	return 0;
}
