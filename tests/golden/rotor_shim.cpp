/* rotor_shim.cpp -- C entry points around the reference's whirl for make_rotor_vectors.py.
 *
 * The generator compiles this file together with the reference's src/whirl.cpp and
 * src/eqcomp.cpp (strict flags, -DCLAP, -I<reference>/src) into a temporary directory, where
 * the reference tree exists; "whirl.h" below is the reference's header and nothing of it is
 * kept here.  whirlProc2 with all six outputs is what the test vectors need and what
 * oracle/_ref/libtbfref.so does not export.
 */
#include "whirl.h"

extern "C" {

/* allocWhirl, the two cfg fields the `levels` case sets on the struct (as oracle/
 * ref_harness.cpp's ref_whirl_cfg does, before initWhirl), initWhirl */
struct b_whirl* rs_new (double sr, int set_levels, double horn_level, double leak_level)
{
	struct b_whirl* w = allocWhirl ();
	if (set_levels) {
		w->hornLevel = horn_level;
		w->leakLevel = leak_level;
	}
	initWhirl (w, nullptr, sr);
	return w;
}

void rs_free (struct b_whirl* w) { freeWhirl (w); }

/* the CLAP setParam mapping of P_DRUM / P_HORN (oracle/ref_harness.cpp ref_set_param) */
void rs_rev_option (struct b_whirl* w, int n) { useRevOption (w, n, 2); }

void rs_bypass (struct b_whirl* w, int on) { w->bypass = on; }

/* the microphone mix whirlProc3 applies: hll hlr dll dlr hrl hrr drl drr */
void rs_mic (const struct b_whirl* w, float* m8)
{
	m8[0] = w->hornMic_hll;
	m8[1] = w->hornMic_hlr;
	m8[2] = w->drumMic_dll;
	m8[3] = w->drumMic_dlr;
	m8[4] = w->hornMic_hrl;
	m8[5] = w->hornMic_hrr;
	m8[6] = w->drumMic_drl;
	m8[7] = w->drumMic_drr;
}

void rs_proc2 (struct b_whirl* w, const float* in, float* L, float* R, float* HL, float* HR, float* DL, float* DR, int n)
{
	whirlProc2 (w, in, L, R, HL, HR, DL, DR, (size_t)n);
}
}
