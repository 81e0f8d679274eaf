/*
 * tbf.h -- C-ABI of the MI355X batched render engine for tuneBfree's DSP chain.
 *
 * Drop-in boundary.  The reference evaluates one organ per plugin instance through
 * four per-block calls issued by synthSound (b_synth/lv2.cpp:212-239,
 * src/clap.cpp:244-270, src/main.cpp:243-292):
 *     oscGenerateFragment (struct b_tonegen*, float* buf, size_t)     src/tonegen.h:594
 *     preamp (void* pa, float* in, float* out, size_t)                 src/overdrive.h:35
 *     b_reverb::reverb (float* in, float* out, int)                    src/reverb.h:30
 *     whirlProc3 (struct b_whirl*, const float*, float*, float*,
 *                 float*, float*, size_t)                              src/whirl.h:245-249
 * tbf_render / tbf_synth_sound replace that quartet for a batch of instances; the
 * control surface replaces the host-side calls that mutate the DSP structs between
 * blocks:
 *     oscKeyOn / oscKeyOff                      src/tonegen.cpp:3096-3166 -> tbf_note
 *     CLAP setParam (drawbars, vibrato, rotary,
 *     overdrive, character, reverb, percussion) src/clap.cpp:162-207     -> tbf_set_param
 *     allocSynth + initSynth                    b_synth/lv2.cpp:336-353, 164-193
 *                                               -> tbf_template_create + tbf_instances_add
 * Event timing is the reference's: anything issued between two render calls takes
 * effect at the next 128-sample block boundary (b_synth/lv2.cpp:1130-1134).
 *
 * Conventions: plain C types, 0 on success, negative errno-style codes on failure
 * (tbf_last_error() has the message); one host thread per engine; no allocation
 * inside tbf_render_device once the instance set is fixed.
 */
#ifndef TBF_H
#define TBF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TBF_ABI_VERSION 1
#define TBF_BLOCK_SAMPLES 128

/* parameter ids: CLAP ids of src/clap.cpp:31-48 ... */
#define TBF_P_DRAWBAR_MIN 0 /* upper manual drawbars 16' .. 1', value 0..8 */
#define TBF_P_DRAWBAR_MAX 8
#define TBF_P_VIBRATO 9            /* upper manual through the scanner, 0/1 */
#define TBF_P_VIBRATO_TYPE 10      /* 0..5 = V1 C1 V2 C2 V3 C3 */
#define TBF_P_DRUM 11              /* 0 stop, 1 slow, 2 fast */
#define TBF_P_HORN 12              /* 0 stop, 1 slow, 2 fast */
#define TBF_P_OVERDRIVE 13         /* 0 clean, 1 overdrive */
#define TBF_P_CHARACTER 14         /* 0..1 */
#define TBF_P_REVERB 15            /* reverb mix 0..1 */
#define TBF_P_PERCUSSION 16        /* 0/1 */
#define TBF_P_PERCUSSION_VOLUME 17 /* 1 normal, 0 soft (CLAP convention) */
#define TBF_P_PERCUSSION_DECAY 18  /* 1 fast, 0 slow */
#define TBF_P_PERCUSSION_HARMONIC 19 /* 1 second (bus A), 0 third (bus B) */
/* ... plus the setters the LV2/JACK hosts reach through MIDI CCs (src/midi.cpp) */
#define TBF_P_BUS_DRAWBAR_BASE 100 /* 100 + bus 0..26 (upper, lower, pedal), value 0..8 */
#define TBF_P_VIBRATO_LOWER 130    /* lower manual through the scanner, 0/1 */
#define TBF_P_SWELL 131            /* swell pedal 0..1 (setSwellPedal1FromMIDI) */
#define TBF_P_WHIRL_BYPASS 132     /* whirl.bypass 0/1 */

#define TBF_CHAIN_FULL 0     /* tonegen -> vibrato -> overdrive -> reverb -> whirl */
#define TBF_CHAIN_TONEGEN 1  /* oscGenerateFragment only, L = R = tonegen output */
#define TBF_CHAIN_TAP_PREAMP 2 /* parity tap: L = R = preamp output */
#define TBF_CHAIN_TAP_REVERB 3 /* parity tap: L = R = reverb output */
/* effects-only chains: the caller's audio instead of the tone generator's, through the
 * tbf_process* calls below (the tbf_render* calls and tbf_synth_sound return -22 on them) */
#define TBF_CHAIN_FX 4            /* caller audio -> overdrive -> reverb -> whirl */
#define TBF_CHAIN_FX_TAP_PREAMP 5 /* parity tap: L = R = preamp output of the caller's audio */
#define TBF_CHAIN_FX_TAP_REVERB 6 /* parity tap: L = R = reverb output */

typedef struct tbf_engine tbf_engine;

/* tbf_engine_config.debug_flags */
#define TBF_DEBUG_FORCE_SERIAL 1u /* fail every fast-path precondition vote, so each guarded
                                   * stage takes its exact serial replay (parity tests of the
                                   * fallbacks; slow) */

/* tbf_engine_config.whirl_out: which of the reference's whirl entry points the engine's L / R
 * are.  The LV2 and CLAP shells call whirlProc3, the JACK host's plain build whirlProc
 * (src/main.cpp:265-281); the two differ in their bits even at the default microphone width
 * (DESIGN.md section 1).  Every call that yields L / R delivers the chosen pair in the same two
 * buffers: tbf_render*, tbf_synth_sound and its FIFO, tbf_process*.  The mode is the engine's,
 * not an instance's: the DSP state is the same in either, so clone, save, load and remove are
 * untouched and a blob saved on an engine of one mode loads into an engine of the other.
 * tbf_engine_create returns -22 for any other value, and for TBF_WHIRL_OUT_DIRECT on a chain
 * that does not run the whirl (TBF_CHAIN_TONEGEN and the tap chains). */
#define TBF_WHIRL_OUT_MIC 0    /* whirlProc3 (src/whirl.cpp:1653-1681): the four rotor signals through the
                                * microphone mix */
#define TBF_WHIRL_OUT_DIRECT 1 /* whirlProc (src/whirl.cpp:1640-1650): whirlProc2's outL / outR, the direct sum
                                * y + hornLevel * H + leak per channel (1592-1606); under bypass the input */

typedef struct tbf_engine_config {
	double   sample_rate; /* Hz, 8000 .. 192000; a chain that runs the whirl (TBF_CHAIN_FULL, TBF_CHAIN_FX)
	                       * needs every rotor write-ahead >= 64 samples: from about 35.5 kHz with the
	                       * default geometry (44100 and up are safe), higher with the microphone nearer
	                       * than the default (whirl.mic.distance under 27 cm at 48 kHz); below that
	                       * tbf_engine_create / tbf_config_set / tbf_config_parse return -22 */
	int32_t  device;      /* HIP device ordinal */
	uint32_t chain_mode;  /* TBF_CHAIN_* */
	uint32_t debug_flags; /* TBF_DEBUG_*, 0 in production */
	uint32_t whirl_out;   /* TBF_WHIRL_OUT_*: what outL / outR of every call carry (the size and layout of the
	                       * struct are those of the three reserved words this field was the first of) */
	uint32_t reserved[2];
} tbf_engine_config;

int         tbf_abi_version (void);
const char* tbf_last_error (void);

int tbf_engine_create (const tbf_engine_config* cfg, tbf_engine** out);
int tbf_engine_destroy (tbf_engine* e);

/* ---- cfg keys (§8(f) row 4): the reference's `key=value` configuration lines ----
 * parseConfigurationLine / distributeParameter (src/cfgParser.cpp:61-160) hand each line
 * to every module; the ones that reach this engine are
 *   whirl.*   whirlConfig (src/whirl.cpp:992-1160): speeds, accelerations, geometry
 *             (horn/drum radius, mic distance, horn offsets), the three filters,
 *             horn level / leak, mic widths and angle, brake positions, speed preset,
 *             bypass.  Geometry re-derives the compact ring window (512 / 1024 / 2048)
 *   scanner.* scannerConfig (src/vibrato.cpp:334-357): scanner frequency, V1-V3 depths
 *   reverb.mix reverbConfig (src/reverb.cpp:242-256)
 *   osc.*     oscConfig (src/tonegen.cpp:2173-2555): x-precision, the key-click /
 *             release envelope models, levels and lengths, percussion gains, buses and
 *             trigger bus (osc.perc.fast / .slow are stored but, as in the reference,
 *             never reach the decay constants); the wheel EQ (osc.eq.macro, spline
 *             points), extra wheel harmonics (osc.harmonic.*), terminal mixes, key tapers
 *             and key crosstalk lists (osc.terminal.* / osc.taper.* / osc.crosstalk.*),
 *             the default crosstalk levels and the contribution floor / minimum
 * A setting applies to what is built after it: whirl.* tables and scanner.* shape
 * engine-wide tables and must precede tbf_instances_add (-16 after); osc.* template
 * keys apply to later tbf_template_create / tbf_templates_create; the rest to later
 * tbf_instances_add.  Returns 0 applied, 1 ignored: not a key of this path, or a key
 * the reference stores but never reads here (overdrive.* / xov.*: ampConfig,
 * src/overdrive.cpp:395-433, writes fields airwindows_density never reads;
 * osc.tuning / osc.temperament / osc.eqv.*; whirl.horn.comb.*), -22 bad value
 * (nothing assigned; a list key with any malformed part assigns none of it, where the
 * reference keeps the well-formed parts and warns; osc.transformer-crosstalk above 0,
 * with which the reference aborts in findTransformerNeighbours,
 * src/tonegen.cpp:914-927). */
int tbf_config_set (tbf_engine* e, const char* key, const char* value);
/* a cfg file's text (`name = value` lines, '#' comments): returns the number of keys
 * applied, or < 0 with tbf_last_error () = "line N: message".  All or nothing: a bad line
 * (or a table-shaping key after tbf_instances_add) applies none of the text's keys. */
int tbf_config_parse (tbf_engine* e, const char* text);

/* Tone-generator template (initToneGenerator's shared tables: wave bank, play matrix,
 * envelopes) for one tuning.  mts128: 128 MTS-ESP note frequencies or NULL for the
 * no-master 12-TET table; ratio9: drawbar target ratios or NULL for
 * {0.5,1.5,1,2,3,4,5,6,8}; seed: srand() seed of the template's rand() stream. */
int tbf_template_create (tbf_engine* e, const double* mts128, const double* ratio9, uint32_t seed,
                         uint32_t* tpl_id);

/* n templates built on the device (replaces n initToneGenerator
 * table builds, src/tonegen.cpp:1470-1630 initOscillators + 2562-2728 initEnvelopes):
 * the same tables as n tbf_template_create calls, with the wave bank's sines and its per-sample rand() draws
 * (each thread jumping the glibc stream to its chunk) computed on the engine's GPU.
 * mts128: n x 128 frequencies or NULL; ratio9: n x 9 or NULL; seeds[n]; ids[n] out.
 * Needs a device engine (-19 on a host-only engine). */
int tbf_templates_create (tbf_engine* e, uint32_t n, const double* mts128, const double* ratio9,
                          const uint32_t* seeds, uint32_t* tpl_ids);

/* Add n instances: instance k uses template tpl_ids[k] and per-instance seed seeds[k]
 * (srand before allocReverb/allocPreamp).  Returns the first new index in *first. */
int      tbf_instances_add (tbf_engine* e, uint32_t n, const uint32_t* tpl_ids, const uint32_t* seeds,
                            uint32_t* first);
uint32_t tbf_instance_count (const tbf_engine* e);

/* MTS-ESP retune (§8(f) row 3): the CLAP plugin's reinitToneGen (src/clap.cpp:129-157,
 * run from process() when MTS_NoteToFrequency or the drawbar ratios change,
 * src/clap.cpp:1133-1175) for instance inst on template tpl_id (built from the new
 * frequencies / ratios with tbf_template_create or tbf_templates_create).  From the next
 * block the instance plays a fresh tone generator on the new tables: no keys down,
 * initToneGenerator's defaults, then drawbars 16'..1', vibrato on/off and vibrato type
 * restored from the instance's CLAP parameter values (their get_info defaults when never
 * set, src/clap.cpp:383-545) and the routing word kept; preamp, reverb and whirl state
 * continue.  Events given after the call apply after the retune, as the reference
 * checks the tuning at the top of process() before the block's events.  The osc.* /
 * scanner.* cfg keys in force now apply to the new tone generator. */
int tbf_instance_retune (tbf_engine* e, uint32_t inst, uint32_t tpl_id);

/* ---- instance state: fork, save, restore ----
 * An instance's complete state -- the device DSP state (reverb rings and predelay history,
 * whirl rings, scanner ring, wheel positions, IIR states, dither streams, rotor angles and
 * ramps, the per-wheel control tables, the current core program) and the host control
 * state -- copied, never re-derived.  The three calls are synchronous and wait for the
 * engine's own stream and the pipelined stage streams; a caller rendering on its own
 * stream must synchronize that stream first (as for tbf_error_flags).
 *
 * tbf_instances_clone appends n instances; new instance *first + k is an exact copy of
 * instance src[k] as it stands now, i.e. as of the next block boundary: the device state,
 * the whole host control state including what is pending and not yet rendered (queued key
 * messages, dirty drawbars / routing, a pending rotary option, whirl parameter set or
 * retune, the control rand() stream) and the source's row of the tbf_synth_sound FIFO.
 * From then on the clone is an ordinary instance: with the same later events it renders
 * the source's samples bit for bit, with other events what the reference renders for an
 * organ of the source's seed with the source's history and then those events.  src may
 * repeat; every src[k] must exist before the call (-22, nothing added); on -12 nothing is
 * added and the existing instances are untouched.  Works on every chain mode, on a
 * host-only engine (device -1: the control plane alone) and before the first render. */
int tbf_instances_clone (tbf_engine* e, uint32_t n, const uint32_t* src, uint32_t* first);
/* The n instances' state into one opaque blob of *size bytes (blob NULL: only the count;
 * otherwise cap must cover it, -22).  A blob is valid for this build of the library only:
 * it is no versioned or portable format, it dumps the engine's structs as they are, and its
 * header (struct sizes, sample rate, chain mode, device / host-only, control path, ring
 * window and slab length, fingerprints of the engine-wide tables and of each instance's
 * template) exists to refuse any other use.  Block granularity: -16 while the
 * tbf_synth_sound FIFO holds unserved frames. */
int tbf_instances_save (tbf_engine* e, uint32_t n, const uint32_t* inst, void* blob, uint64_t cap, uint64_t* size);
/* Overwrites the existing, distinct instances inst[k] with the blob's k-th record (inst need
 * not be the indices saved from): on the same engine (rewind) or on another engine created
 * with the same configuration and holding an equal template at the same id (migrate).  n
 * must equal the blob's count and every header field and fingerprint must match, else -22
 * with tbf_last_error () naming the first mismatch; every length in the blob is checked
 * against size (a truncated or corrupted blob is a -22, never an out-of-range read), and
 * everything is validated before anything is touched: a failed load changes nothing.
 * -16 while the tbf_synth_sound FIFO holds unserved frames. */
int tbf_instances_load (tbf_engine* e, uint32_t n, const uint32_t* inst, const void* blob, uint64_t size);
/* Removes the n distinct existing instances inst[0..n) and gives their memory back.  The
 * survivors keep their relative order and are renumbered densely, like a vector after an
 * erase: a survivor's new index is its old index minus the number of removed instances
 * below it, and tbf_instance_count drops by n.  new_index may be NULL; otherwise it has room
 * for the old instance count, and on success new_index[i] is the new index of old instance
 * i, or UINT32_MAX if it was removed.
 * A survivor's state is copied, never re-derived, the same contract as a clone: every later
 * sample is bit-identical to what it would have rendered had the call never been made.  That
 * covers its device DSP state, its whole host control state including what is pending and
 * not yet rendered (queued key messages, dirty drawbars / routing, a pending rotary option,
 * whirl parameter set or retune, the control rand() stream), its persistent program slot
 * rotation and its row of the tbf_synth_sound FIFO (frames pending there are no -16 case:
 * the rows are compacted like every other per-instance array).  Nothing of a removed
 * instance remains, its pending events and its pending retune included.  Templates are
 * untouched and template ids stay valid.
 * -22 if an index does not exist or is listed twice, or if inst is NULL with n > 0; n == 0
 * is a successful no-op (new_index: the identity); -12 on out of memory, -5 if the mover
 * fails.  Everything is validated before anything is touched, and on any failure nothing
 * changes: count, indices, device state and host state are as before.  Removing every
 * instance is allowed: the engine then renders nothing (returns 0) and takes
 * tbf_instances_add again; the table-shaping cfg keys stay refused (-16) once any instance
 * has ever been added.
 * On the device the survivors are compacted into fresh arrays sized for the new count by one
 * k_state_move pass, and the old arrays are released only after it has finished, so the
 * transient peak is the old state plus the new state (about 343 KB per survivor: 1.4 GB
 * extra when a few of 4096 are removed).  The stage buffers are released with the call and
 * come back, for the new count, at the next render.  Synchronisation as for a clone.  Works
 * on every chain mode, on both control paths and front ends, on a host-only engine (device
 * -1: the control plane alone) and before the first render. */
int tbf_instances_remove (tbf_engine* e, uint32_t n, const uint32_t* inst, uint32_t* new_index);

int tbf_note (tbf_engine* e, uint32_t inst, int32_t key, int32_t on);
int tbf_set_param (tbf_engine* e, uint32_t inst, int32_t param, double value);

/* Render nblocks x 128 samples for every instance.  Host buffers; instance i writes
 * out[i * stride + 0 .. nblocks*128).  Synchronous. */
int tbf_render (tbf_engine* e, uint32_t nblocks, float* outL, float* outR, uint64_t stride);

/* Same into device memory on `stream` (hipStream_t, NULL = the engine's own
 * non-blocking stream); returns once the work is enqueued.  Outputs stay in HBM.
 * Ordering: the render is ordered after earlier work on `stream` and the outputs are
 * complete when `stream` reaches this point.  A NULL stream is NOT the legacy default
 * stream: a caller that consumes the outputs on another stream (e.g. torch's current
 * stream, whose handle is 0 on the default stream) must pass that stream's real handle
 * or call tbf_synchronize () first.
 * stride and pointers need only float alignment: the kernels store the outputs one float
 * at a time, so any stride >= nblocks*128 (odd ones included) and any 4-byte-aligned
 * d_outL / d_outR are valid, and nothing outside [0, nblocks*128) of a row is written. */
int tbf_render_device (tbf_engine* e, uint32_t nblocks, float* d_outL, float* d_outR, uint64_t stride,
                       void* stream);

/* synthSound semantics (b_synth/lv2.cpp:212-239): serve nframes per instance out of
 * the 128-sample block FIFO, rendering blocks as needed.  Instance i writes
 * out[i * stride + 0 .. nframes); stride >= nframes (else -22). */
int tbf_synth_sound (tbf_engine* e, uint32_t nframes, float* outL, float* outR, uint64_t stride);

/* ---- host control surface (src/midi.cpp, src/program.cpp, src/pgmParser.cpp) ---- */
/* callMIDIControlFunction (src/midi.cpp:535-545) on one instance.  fn is a control
 * function name of src/midi.cpp:100-170 that reaches the DSP chain: upper|lower|pedal.
 * drawbar16/513/8/4/223/2/135/113/1, percussion.enable|volume|decay|harmonic,
 * vibrato.knob|routing|upper|lower, swellpedal1|2, overdrive.enable|character,
 * reverb.mix, rotary.speed-preset|speed-select|speed-toggle, and the whirl's
 * whirl.horn.filter.a|b.type|hz|q|gain, whirl.horn|drum.brakepos,
 * whirl.horn|drum.acceleration|deceleration (src/whirl.cpp:699-889, registered 966-981;
 * from the next block), and convolution.mix (src/midi.cpp:168; the cabinet calls' mix,
 * below).  value 0..127 (clamped).  Returns 0 when applied, 1 for any
 * other name (ignored, as the reference ignores names without a registered function). */
int tbf_midi_control (tbf_engine* e, uint32_t inst, const char* fn, int32_t value);
/* programme definitions in the .pgm syntax (src/pgmParser.cpp:65-73, properties of
 * bindToProgram src/program.cpp:133-603) into the engine's programme table; returns the
 * number of programmes in use, or < 0 with tbf_last_error () = "line N: message" */
int tbf_program_parse (tbf_engine* e, const char* text);
/* installProgram (src/program.cpp:735-921): MIDI program change pc (0..127, plus the
 * reference's default pgm.controller.offset of 1) on one instance; random drawbars draw
 * from the instance's control rand() stream */
int tbf_program_install (tbf_engine* e, uint32_t inst, uint32_t pc);
/* name of the programme program change pc selects; returns 1 if in use, else 0 */
int tbf_program_name (tbf_engine* e, uint32_t pc, char* out, uint32_t cap);

/* ---- scheduled events (§8(f) row 1): a whole event script in one render ---- */
#define TBF_EV_NOTE 0    /* id = key 0..383 (oscKeyOn/Off), value != 0: on */
#define TBF_EV_PARAM 1   /* id = TBF_P_*, value as tbf_set_param */
#define TBF_EV_CONTROL 2 /* id = tbf_midi_control_id (name), value 0..127 */
#define TBF_EV_PROGRAM 3 /* id = program change 0..127 (tbf_program_install) */

typedef struct tbf_event {
	uint32_t block; /* block index (from the start of this call) before which it applies */
	uint32_t inst;
	int32_t  kind;  /* TBF_EV_* */
	int32_t  id;
	double   value;
} tbf_event;

/* id of a control function name for TBF_EV_CONTROL events, < 0 if not a hot-path name */
int tbf_midi_control_id (const char* fn);
/* render nblocks with events applied at their block boundaries (b_synth/lv2.cpp:
 * 1130-1134 timing), into device memory like tbf_render_device.  Events must be sorted
 * by block; within a block they apply in array order; events at or beyond nblocks apply
 * after the render.  The host steps the control plane per block and uploads only the
 * per-block control deltas, so one launch set covers a whole chunk of 64 blocks however
 * many events land in it. */
int tbf_render_events (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, float* d_outL,
                       float* d_outR, uint64_t stride, void* stream);

/* ---- effects-only chains (TBF_CHAIN_FX*): the caller's audio through the effects ----
 * preamp -> b_reverb::reverb -> whirlProc3 of the reference on caller-supplied mono audio,
 * one row per instance, with the instance's own effect state (the same srand (seed) ->
 * allocReverb -> allocPreamp as a full-chain instance of that seed) and control surface:
 * tbf_set_param, tbf_midi_control, cfg keys and events act as on the full chain, and what
 * faces the tone generator (notes, drawbars, vibrato, percussion, programmes, retune) is
 * accepted and inaudible.  The tone generator never runs and has no stage buffer.
 * Instance i reads in[i * in_stride + 0 .. nblocks*128); in_stride >= nblocks*128, odd
 * strides and any 4-byte-aligned pointer are valid, and nothing outside [0, nblocks*128) of a
 * row is read.  Inputs are finite floats; subnormals and -0.f pass as through the
 * reference.  The input range must not overlap either output range (-22).  Events apply at
 * block boundaries, as in tbf_render_events (no frame-granular FIFO: tbf_synth_sound has no
 * counterpart here).  On an engine of another chain mode these calls return -22, on a
 * host-only engine of an effects-only chain -19. */
/* host buffers, synchronous */
int tbf_process (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t in_stride, float* outL, float* outR,
                 uint64_t stride);
/* device memory on `stream`, as tbf_render_device, and the same ordering extended to the
 * input: d_in must be complete when `stream` reaches this call (the first stage of every
 * call waits for `stream`), and may be overwritten once `stream` has passed it */
int tbf_process_device (tbf_engine* e, uint32_t nblocks, const float* d_in, uint64_t in_stride, float* d_outL,
                        float* d_outR, uint64_t stride, void* stream);
/* the same with events, as tbf_render_events */
int tbf_process_events (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* d_in,
                        uint64_t in_stride, float* d_outL, float* d_outR, uint64_t stride, void* stream);

/* ---- rotor outputs: whirlProc2's horn and drum pairs out of one render ----
 * The reference's JACK host in its cabinet-convolution build calls whirlProc2 (w, in, NULL,
 * NULL, hornL, hornR, drumL, drumR, n), sends the horn pair through its convolver and mixes the
 * drum pair in afterwards (src/main.cpp:265-281).  These calls deliver the four signals of one
 * render: hornL / hornR = hornLevel * H + leak and drumL / drumR = the drum shelves' outputs,
 * exactly whirlProc2's outHL / outHR / outDL / outDR (src/whirl.cpp:1592-1606); under bypass
 * the horn pair is the input and the drum pair 0 (1197-1215).  Instance i writes plane[i *
 * rotors->stride + 0 .. nblocks*128) of each of the four planes; all four pointers are required,
 * rotors->stride >= nblocks*128, and for device memory the tbf_render_device contract holds
 * (float alignment, odd strides, nothing outside [0, nblocks*128) of a row is written).  outL /
 * outR carry what the engine's whirl_out says, at their own stride, or are both NULL.  The
 * output ranges must not overlap one another.
 * -22 on a chain that does not run the whirl, on a missing pointer (rotors, one of its four,
 * one of outL / outR without the other), on a short stride and on an effects-only input range
 * that overlaps any of the six outputs; -19 on a host-only engine.  Validation comes first: a
 * refused call renders nothing and steps no control.  tbf_debug_launches counts these renders'
 * whirl launches as TBF_LAUNCH_WHIRL / TBF_LAUNCH_WHIRL_SPLIT.  There is no frame-granular FIFO
 * for the rotor planes: a host that serves odd frame counts keeps its own (as for
 * tbf_process*). */
typedef struct tbf_rotor_out {
	float*   hornL; /* hornLevel * H + leak, left and right (outHL, outHR) */
	float*   hornR;
	float*   drumL; /* the drum shelves' outputs (outDL, outDR) */
	float*   drumR;
	uint64_t stride; /* floats between instances, the same for the four planes */
} tbf_rotor_out;
/* TBF_CHAIN_FULL; host buffers, synchronous (as tbf_render) */
int tbf_render_rotors (tbf_engine* e, uint32_t nblocks, float* outL, float* outR, uint64_t stride,
                       const tbf_rotor_out* rotors);
/* TBF_CHAIN_FULL; device memory on `stream` with events, as tbf_render_events (ev == NULL with
 * nev == 0: no events, as tbf_render_device) */
int tbf_render_rotors_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, float* d_outL,
                              float* d_outR, uint64_t stride, const tbf_rotor_out* rotors, void* stream);
/* TBF_CHAIN_FX; host buffers, synchronous (as tbf_process) */
int tbf_process_rotors (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t in_stride, float* outL,
                        float* outR, uint64_t stride, const tbf_rotor_out* rotors);
/* TBF_CHAIN_FX; device memory on `stream` with events, as tbf_process_events */
int tbf_process_rotors_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* d_in,
                               uint64_t in_stride, float* d_outL, float* d_outR, uint64_t stride,
                               const tbf_rotor_out* rotors, void* stream);

/* ---- cabinet convolver: the horn pair through an impulse response, on the device ----
 * The last stage of the reference's JACK host in its convolver build (src/main.cpp:265-281):
 * whirlProc2, then the horn pair through the convolver, then the drum pair mixed in.  The
 * reference tree holds the call site and the control name but not the convolver, so the
 * arithmetic and the mix law below are this project's own definition.
 * Cabinet: one engine-wide stereo impulse response at the engine's sample rate, irL[taps] and
 * irR[taps]; hornL is convolved with irL and hornR with irR, no cross terms.  Per instance,
 * channel and sample
 *     wet_n = sum_k ir[k] * horn[n-k]      (horn before the instance's first cabinet block = 0;
 *                                           no added latency)
 *     out_n = (dry * horn_n + mix * wet_n) + drum_n,   dry = 1.0f - mix
 * where every operation of the second line is one float32 operation in that association, and
 * horn / drum are what the tbf_*_rotors* calls deliver (under whirl.bypass: the input and 0).
 * The convolution is a partitioned FFT convolution in float32 (csrc/tbf_cabinet.hip); against a
 * float64 direct sum its error stays within a few 2^-24 of max|horn| * sum|ir|.
 * mix is per instance, 1.0f unless set: by the cfg key convolution.mix (0..1, for instances
 * added afterwards), by tbf_midi_control (inst, "convolution.mix", v): mix = (float)(v / 127.0),
 * or by a TBF_EV_CONTROL event with that name's id; like every control it takes effect at the
 * next block boundary.  It is stored (and returns 0) on every engine, with or without a cabinet,
 * and is part of the host control state that clone, save, load and remove carry.
 * State: per instance and channel the spectra of the last horn blocks, zero at
 * tbf_instances_add.  It advances only through the cabinet calls: a tbf_render*, tbf_process* or
 * tbf_*_rotors* call in between renders blocks the convolver never hears, so a host uses one
 * family of calls.  It is instance state: clone, save, load and remove copy it; a blob's header
 * carries the response's length and a fingerprint of its taps, and a load into an engine with
 * another cabinet, or none, returns -22 ("cabinet ..."); tbf_debug_device_bytes counts it.
 * Like every render, the cabinet planes of a block are bit-identical however the render is cut
 * into calls and chunks and whether controls come by call or by event. */
#define TBF_CAB_MAX_TAPS 8192
/* engine-wide; shapes per-instance state, so before the first tbf_instances_add (-16 after).  -22: NULL ir with
 * taps > 0, taps > TBF_CAB_MAX_TAPS, a non-finite tap, a chain that does not run the whirl.  taps == 0: no cabinet. */
int tbf_cabinet_set (tbf_engine* e, const float* irL, const float* irR, uint32_t taps);
typedef struct tbf_cabinet_out {
	float*   L;    /* required: (dry * horn + mix * wet) + drum */
	float*   R;
	float*   wetL; /* both or neither: the convolver's own output */
	float*   wetR;
	uint64_t stride; /* floats between instances, the same for the planes given */
} tbf_cabinet_out;
/* tbf_render_cabinet* for TBF_CHAIN_FULL, tbf_process_cabinet* for TBF_CHAIN_FX; host buffers and
 * synchronous, or device memory on `stream` with events, as the tbf_*_rotors* calls.  rotors may
 * be NULL; otherwise all four of its planes are required and receive the call's rotor signals.
 * Without rotors the engine renders them into scratch of its own, at most 16 B per instance and
 * sample of 256 blocks (a longer call is cut into pieces), -12 when the device cannot hold it.
 * -22 without a cabinet, on the wrong chain, on a missing pointer or half a pair, on a short
 * stride, and when any two of the ranges (input, cabinet planes, rotor planes) overlap; -19 on a
 * host-only engine.  Validation comes first: a refused call renders nothing, steps no control
 * and moves no history.  Device memory follows tbf_render_device's contract (float alignment,
 * odd strides, nothing outside [0, nblocks*128) of a row written).  No frame-granular FIFO. */
int tbf_render_cabinet (tbf_engine* e, uint32_t nblocks, const tbf_cabinet_out* cab, const tbf_rotor_out* rotors);
int tbf_render_cabinet_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev,
                               const tbf_cabinet_out* cab, const tbf_rotor_out* rotors, void* stream);
int tbf_process_cabinet (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t in_stride, const tbf_cabinet_out* cab,
                         const tbf_rotor_out* rotors);
int tbf_process_cabinet_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* d_in,
                                uint64_t in_stride, const tbf_cabinet_out* cab, const tbf_rotor_out* rotors, void* stream);
/* test hook: taps, partitions K, history bytes per instance, k_cabinet launches so far, and one instance's mix
 * (any pointer may be NULL; inst is checked only with wet) */
int tbf_debug_cabinet (const tbf_engine* e, uint32_t inst, uint32_t* taps, uint32_t* parts, uint64_t* inst_bytes,
                       uint64_t* launches, float* wet);

/* k_cabinet's own time, with HIP events around each launch on its stream: enable 1 / -1 turns recording on / off;
 * 0 returns the summed milliseconds and the launches since the last query (it waits for them) */
int tbf_debug_cabinet_time (tbf_engine* e, int32_t enable, double* ms, uint64_t* launches);

/* ---- output rate conversion: L / R at another sample rate, on the device ----
 * A streaming polyphase rate converter behind whatever L / R the chain and whirl_out deliver, on
 * every chain mode.  Like the cabinet it is specified here, not restated from the reference
 * (DESIGN.md section 7): the reference renders at its host's rate only, and at another rate it
 * renders other audio (its whirl geometry is in samples).
 * The engine rate Fi must be an integer number of Hz; the output rate Fo is an integer number of
 * Hz and differs from Fi.  L / M = Fo / Fi in lowest terms.
 * Prototype filter, built once on the host in double and rounded to float32:
 *     s = max (L, M);  Z = 32 zero crossings a side;
 *     T = ceil (2 Z s / L), rounded up to even: the taps per phase;  N = L T;  c = (N - 1) / 2;
 *     fc = 0.45 / s  (0.9 of the narrower Nyquist);
 *     g[k] = L * 2 fc * sinc (2 fc (k - c)) * kaiser (k; N, beta = 10),   k = 0 .. N - 1,
 *     sinc (x) = sin (pi x) / (pi x), the Kaiser window with a double-precision I0 series.
 * Position: per instance, P (uint64) counts the engine-rate samples the converter has consumed
 * since tbf_instances_add; x[j] is the instance's L (or R) sample number j, x[j < 0] = 0.
 * Output count: output sample n exists once n M < P L, so C (P) = ceil (P L / M) outputs exist
 * after P inputs.  A call that feeds nblocks * 128 samples delivers exactly the outputs
 * n in [C (P), C (P + nblocks * 128)) of each instance; each has P <= floor (n M / L) < P + nblocks * 128.
 * Arithmetic, per output n:  p = n M in 64 bits, i = p div L, phi = p mod L,  acc = 0.0f,
 *     for t = 0 .. T - 1 ascending:  acc = fmaf (g[phi + t L], x[i - t], acc);     y[n] = acc,
 * each step one float32 fmaf, denormals kept.  Nothing depends on call or chunk length, so the
 * output is bit-identical at every cut into calls, chunks and scratch pieces, and whether
 * controls come by call or by event.
 * The latency is (N - 1) / (2 L) engine-rate samples; it is reported, not compensated.  Counts
 * differ between instances whenever their P differ (an instance added later, a blob loaded from
 * another time).  The cap: L <= 1024 and L T <= 2^18.
 * State: on the device the last T - 1 inputs per instance and channel, zero at
 * tbf_instances_add; on the host P per instance.  It advances only through the calls below: a
 * tbf_render*, tbf_process*, rotor or cabinet call in between renders blocks the converter never
 * hears, so a host uses one family of calls.  It is instance state: clone copies it (P
 * included), save / load copy it (the blob header carries Fo, L, M, T and a fingerprint of the
 * table; a load into an engine with another converter, or none, returns -22 "resampler ..."),
 * remove compacts it; tbf_debug_device_bytes counts it when a converter is set. */
/* engine-wide; shapes per-instance state, so before the first tbf_instances_add (-16 after).  0: no converter.
 * -22: a non-integer engine rate, out_rate_hz equal to the engine's rate, a ratio beyond the cap. */
int tbf_resampler_set (tbf_engine* e, uint32_t out_rate_hz);
/* ceil (nblocks * 128 * L / M): the bound on any instance's count for such a call, and the least output stride accepted */
int tbf_resampled_frames (const tbf_engine* e, uint32_t nblocks, uint64_t* max_frames);
typedef struct tbf_resampled_out {
	float*    L;    /* required: the converted pair; instance i gets [0, counts[i]) of its rows */
	float*    R;
	float*    rawL; /* both or neither: the engine-rate pair, bit-identical to tbf_render_device's */
	float*    rawR;
	uint64_t  stride;     /* floats between instances of L / R: at least tbf_resampled_frames (nblocks) */
	uint64_t  raw_stride; /* floats between instances of rawL / rawR: at least nblocks * 128 */
	uint32_t* counts;     /* required, host memory, one per instance: filled before the call returns */
} tbf_resampled_out;
/* tbf_render_resampled* for TBF_CHAIN_FULL, TBF_CHAIN_TONEGEN and the tap chains, tbf_process_resampled*
 * for the TBF_CHAIN_FX* chains; host buffers and synchronous, or device memory on `stream` with
 * events, as the cabinet calls.  counts is host memory in both forms: the host owns P, so the
 * counts are known without waiting for the device.  Without the raw planes the engine renders
 * L / R into scratch of its own, at most 8 B per instance and sample of 256 blocks (a longer call is
 * cut into pieces, each with its own events), -12 before anything renders when the device cannot
 * hold it.  -22 without a converter, with the wrong family for the chain, on a missing pointer or
 * half a pair, on a short stride, when any two of the ranges (input, converted rows over
 * tbf_resampled_frames, raw rows) overlap, and for a call whose counts would pass 32 bits; -19
 * on a host-only engine.  Validation comes first: a refused call renders nothing, steps no
 * control and moves no state.  Device memory follows tbf_render_device's contract (float
 * alignment, odd strides); nothing outside [0, counts[i]) of a converted row and
 * [0, nblocks*128) of a raw row is written. */
int tbf_render_resampled (tbf_engine* e, uint32_t nblocks, const tbf_resampled_out* out);
int tbf_render_resampled_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev,
                                 const tbf_resampled_out* out, void* stream);
int tbf_process_resampled (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t in_stride,
                           const tbf_resampled_out* out);
int tbf_process_resampled_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* d_in,
                                  uint64_t in_stride, const tbf_resampled_out* out, void* stream);
/* test hook: L, M, T, the float32 table g[k] in k order (table may be NULL; -22 when cap < L T) and the latency in
 * engine-rate samples; works on a host-only engine; zeros without a converter */
int tbf_debug_resampler (const tbf_engine* e, uint32_t* L, uint32_t* M, uint32_t* T, float* table, uint64_t cap,
                         double* latency);
/* test hook: the host restatement of the definition on one row, from the header the kernel is built from
 * (csrc/tbf_resample.h) with libm's fmaf.  x holds the n_in samples pos0 .., hist the T - 1 samples before them (NULL:
 * zeros); y receives the outputs [C (pos0), C (pos0 + n_in)), *n_out their number (-22 when cap is smaller).  Works on
 * a host-only engine. */
int tbf_debug_resample_ref (const tbf_engine* e, const float* x, uint64_t n_in, const float* hist, uint64_t pos0, float* y,
                            uint64_t cap, uint64_t* n_out);
/* test hook: sets an instance's P and leaves its history alone (tests place n M across 2^32 with it) */
int tbf_debug_resampler_pos (tbf_engine* e, uint32_t inst, uint64_t pos);
/* k_resample's own time, as tbf_debug_cabinet_time */
int tbf_debug_resample_time (tbf_engine* e, int32_t enable, double* ms, uint64_t* launches);

/* ---- PCM output: interleaved integer frames with meters, on the device ----
 * A last stage behind any two float32 planes: whatever L / R the chain and whirl_out deliver, or
 * (tbf_pcm_convert_device) any pair of device planes, the converted rows of the resampled calls
 * and the cabinet and rotor planes included.  It turns them into the interleaved frames a WAV
 * writer, a dataset shard or an audio sink takes, and meters them on the way.  Like the cabinet
 * and the rate converter it is specified here, not restated from the reference (DESIGN.md section
 * 7).  It has no instance state: clone, save, load and remove do not know it.
 * A frame is L then R, little-endian, frames back to back; row r holds its frames from byte
 * r * out_stride_bytes of `out`.
 * Quantisation, per float32 sample x, with S = 32768.0f (S16) or 8388608.0f (S24), denormals kept:
 *     v = x * S                         one float32 multiply
 *     t = v, or with dither t = v + d   one float32 add
 *     q = rintf (t)                     ties to even
 *     NaN: q = 0;   q > max: q = max;   q < min: q = min;   each counted as a clip
 *     max = 32767 / 8388607,  min = -32768 / -8388608.
 * So x = 1.0f clips to max (and is counted): full scale is [-1, 1 - 1 / S].  TBF_PCM_F32 copies
 * the sample's bits unchanged (-0.f, subnormals and NaN payloads included) and counts a clip where
 * !(fabsf (x) <= 1.0f).
 * Dither (TBF_PCM_DITHER, S16 only: -22 with another format) is TPDF of +-1 LSB, counter-based and
 * stateless.  With h (a) the 32-bit mixer
 *     a ^= a >> 16;  a *= 0x7feb352d;  a ^= a >> 15;  a *= 0x846ca68b;  a ^= a >> 16
 * the sample of row r, channel c (0: L, 1: R) and 64-bit frame index f = frame0 (r) + j, j the
 * frame's place in the call's row, gets
 *     k = h (h (h (seed ^ (2 r + c)) ^ lo32 (f)) ^ hi32 (f))
 *     d = ((float)(k & 0xffff) - (float)(k >> 16)) * 0x1p-16f.
 * seed and frame0 are the caller's; dither is no instance state.  A caller who passes the frames
 * delivered so far as frame0 gets the same bytes at every cut into calls.  The row number is the
 * instance's index, so tbf_instances_remove, which renumbers the survivors, changes their dither
 * stream from then on (a caller who minds keeps its own numbering in seed and row_frame0).
 * Meters, optional, one per row: peak = the largest fabsf (x) of the row's frames in this call
 * (NaN skipped; 0 for an empty row), clip = the count above.  Each call overwrites them; they do
 * not accumulate across calls.  Both are independent of order, so they are exact. */
#define TBF_PCM_S16 0u     /* int16 L, int16 R: 4 B per frame */
#define TBF_PCM_S24_3LE 1u /* packed 3-byte little-endian L, R: 6 B per frame */
#define TBF_PCM_F32 2u     /* float32 L, R: 8 B per frame */
#define TBF_PCM_DITHER 1u  /* tbf_pcm_out.flags */
typedef struct tbf_pcm_meter {
	float    peakL, peakR;
	uint32_t clipL, clipR;
} tbf_pcm_meter;
typedef struct tbf_pcm_out {
	void*           out;              /* required; 4-byte aligned in the *_device calls */
	uint64_t        out_stride_bytes; /* bytes between rows: a multiple of 4, at least frames * frame bytes */
	tbf_pcm_meter*  meters;           /* optional, one per row: device memory in the *_device calls, host memory in the host calls */
	uint32_t        format;           /* TBF_PCM_S16 / _S24_3LE / _F32 */
	uint32_t        flags;            /* 0 or TBF_PCM_DITHER */
	uint32_t        seed;             /* dither */
	uint64_t        frame0;           /* dither: the frame index of every row's first frame ... */
	const uint64_t* row_frame0;       /* ... or, optional, host memory, one per row: each row's own */
} tbf_pcm_out;
/* The stage alone: n_rows rows of d_L / d_R (device memory, row r at r * in_stride floats; any
 * 4-byte-aligned pointers and odd strides, as tbf_render_device delivers them; d_L == d_R is
 * allowed) into out->out on `stream` (NULL: the engine's own), ordered as tbf_render_device: the
 * planes must be complete where `stream` reaches the call, the frames and meters are complete
 * when it has passed it.  Row r converts counts[r] frames (counts: host memory, each <= frames),
 * or `frames` when counts is NULL; n_rows need not be the instance count.  Nothing outside
 * [0, count * frame bytes) of a row is written.  With counts or row_frame0 the call waits for
 * their upload before it returns.  An engine's PCM calls share staging: calls on different
 * streams are the caller's to order. */
int tbf_pcm_convert_device (tbf_engine* e, uint32_t n_rows, const float* d_L, const float* d_R, uint64_t in_stride,
                            uint32_t frames, const uint32_t* counts, const tbf_pcm_out* out, void* stream);
/* One render (tbf_render_pcm* for TBF_CHAIN_FULL, TBF_CHAIN_TONEGEN and the tap chains) or
 * effects-only pass (tbf_process_pcm* for the TBF_CHAIN_FX* chains) delivered as nblocks * 128
 * frames per instance, row = instance: host buffers and synchronous, or device memory on `stream`
 * with events, as the cabinet and resampled calls.  The L / R behind them are tbf_render_device's,
 * bit for bit.  The engine renders them into scratch of its own, at most 8 B per instance and
 * sample of 256 blocks; a longer call is cut into pieces, each with its own events, and delivers
 * the bytes and meters of one call.  The host forms convert into device staging and copy the
 * packed rows out once per piece.  -12 before anything renders when the device cannot hold the
 * scratch.
 * -22: a format or flag that does not exist, dither with another format than S16, a missing
 * pointer, out_stride_bytes no multiple of 4 or smaller than the row, a misaligned device
 * pointer, a count above frames, ranges that overlap (input, frames, meters), the wrong family
 * for the chain, events out of order; -19 on a host-only engine.  Validation comes first: a
 * refused call renders nothing and steps no control. */
int tbf_render_pcm (tbf_engine* e, uint32_t nblocks, const tbf_pcm_out* out);
int tbf_render_pcm_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const tbf_pcm_out* out,
                           void* stream);
int tbf_process_pcm (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t in_stride, const tbf_pcm_out* out);
int tbf_process_pcm_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* d_in,
                            uint64_t in_stride, const tbf_pcm_out* out, void* stream);
/* test hook: the host restatement of the definition on one row, from the header the kernel is
 * built from (csrc/tbf_pcm.h): n frames of L / R as row `row` from dither frame frame0 into
 * n * frame bytes of out and (optional) one meter.  Needs no engine and no device.  -22 as above. */
int tbf_debug_pcm_ref (uint32_t format, uint32_t flags, uint32_t seed, uint32_t row, uint64_t frame0, const float* L,
                       const float* R, uint64_t n, void* out, tbf_pcm_meter* meter);
/* k_pcm's own time, as tbf_debug_cabinet_time */
int tbf_debug_pcm_time (tbf_engine* e, int32_t enable, double* ms, uint64_t* launches);

/* ---- Mixdown: groups of rows summed to stereo buses, on the device ----
 * A stage behind any two float32 planes, stateless: whatever L / R the chain and whirl_out
 * deliver, or (tbf_mix_device) any pair of device planes, the converted rows of the resampled
 * calls and the cabinet and rotor planes included.  It sums groups of rows into stereo buses in a
 * defined order, so a mix is as reproducible as the planes behind it, and it writes planes that
 * tbf_pcm_convert_device takes as they come.  Like the cabinet, the rate converter and the PCM
 * stage it is specified here, not restated from the reference.  It has no
 * instance state: clone, save, load and remove do not know it.
 * Input: n_rows rows of d_L / d_R.  Row r starts at r * in_stride floats.  Row r holds
 * counts[r] <= frames valid frames, or `frames` when counts is NULL.
 * Per row, a tbf_mix_row { uint32_t bus; float ll, lr, rl, rr; }.  bus == TBF_MIX_NONE
 * (UINT32_MAX) means the row is in no bus: not one byte of it is read.  Otherwise bus < n_buses.
 * Output: n_buses rows of outL / outR, each of exactly `frames` frames.
 * For bus b and frame j, visit the rows r in ascending r with bus[r] == b and j < count[r].  Each
 * line is one float32 fmaf, in this order:
 *     accL = accR = +0.0f
 *     for each such row r:
 *         accL = fmaf (ll_r, L_r[j], accL);  accL = fmaf (lr_r, R_r[j], accL);
 *         accR = fmaf (rl_r, L_r[j], accR);  accR = fmaf (rr_r, R_r[j], accR);
 *     outL[b][j] = accL;  outR[b][j] = accR
 * Denormals are kept.  NaN and Inf propagate literally.  No term is skipped because a coefficient
 * is zero: only TBF_MIX_NONE and j >= count[r] remove a term.  A bus with no member, and the
 * frames of a bus that none of its members reaches, are +0.0f.  d_L == d_R is allowed (mono
 * planes).  Nothing here depends on call or chunk length, so a bus's bits are the same however a
 * render is cut.  The order is part of the definition: the kernel parallelises over buses and
 * frames, never over one bus's rows, and uses no float atomics. */
#define TBF_MIX_NONE 0xFFFFFFFFu /* tbf_mix_row.bus: the row is in no bus */
typedef struct tbf_mix_row {
	uint32_t bus;            /* TBF_MIX_NONE, or < n_buses */
	float    ll, lr, rl, rr; /* finite: L -> busL, R -> busL, L -> busR, R -> busR */
} tbf_mix_row;
typedef struct tbf_mix_out {
	float*   L;      /* n_buses rows, bus b from b * stride floats: device memory in the *_device calls and */
	float*   R;      /* tbf_mix_device (4-byte aligned), host memory in the host calls */
	uint64_t stride; /* floats between rows, >= frames */
} tbf_mix_out;
/* The stage alone: n_rows rows of d_L / d_R (device memory; any 4-byte-aligned pointers and odd
 * strides, as tbf_render_device delivers them) into out->L / out->R on `stream` (NULL: the
 * engine's own), ordered as tbf_render_device: the planes must be complete where `stream` reaches
 * the call, the buses are complete when it has passed it.  Nothing outside [0, frames) of an
 * output row is written.  n_rows need not be the instance count.  rows and counts are host
 * memory: the call turns them into a bus-sorted list and waits for its upload before it returns.
 * n_buses has no cap beyond memory.  An engine's mix calls share staging: calls on different
 * streams are the caller's to order. */
int tbf_mix_device (tbf_engine* e, uint32_t n_rows, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames,
                    const uint32_t* counts, const tbf_mix_row* rows, uint32_t n_buses, const tbf_mix_out* out, void* stream);
/* One render (tbf_render_mix* for TBF_CHAIN_FULL, TBF_CHAIN_TONEGEN and the tap chains) or
 * effects-only pass (tbf_process_mix* for the TBF_CHAIN_FX* chains) delivered as n_buses rows of
 * nblocks * 128 frames, row r of `rows` = instance r: host buffers and synchronous, or device
 * memory on `stream` with events, as the PCM calls.  The L / R behind them are
 * tbf_render_device's, bit for bit.  The engine renders them into scratch of its own, at most
 * 8 B per instance and sample of 256 blocks; a longer call is cut into pieces, each with its own
 * events, each mixed at its frame offset, and delivers the bits of one call.  The host forms mix
 * into device staging and copy the buses out once per piece; their rows and out are host memory.
 * -12 before anything renders when the device cannot hold the scratch.
 * -22, with a tbf_last_error that names the argument: a NULL pointer, n_buses == 0 while a row
 * names a bus, a bus index >= n_buses, a non-finite coefficient of a row in a bus, a stride
 * smaller than the row, a misaligned device pointer, counts[r] > frames, any overlap among the
 * input rows, the two output planes and the effects-only input (each taken as one range from its
 * first row's first frame to its last row's last), the wrong family for the chain, events out of
 * order; -19 on a host-only engine.  Validation comes first: a refused call renders nothing,
 * steps no control and writes nothing. */
int tbf_render_mix (tbf_engine* e, uint32_t nblocks, const tbf_mix_row* rows, uint32_t n_buses, const tbf_mix_out* out);
int tbf_render_mix_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const tbf_mix_row* rows,
                           uint32_t n_buses, const tbf_mix_out* out, void* stream);
int tbf_process_mix (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t in_stride, const tbf_mix_row* rows,
                     uint32_t n_buses, const tbf_mix_out* out);
int tbf_process_mix_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* d_in,
                            uint64_t in_stride, const tbf_mix_row* rows, uint32_t n_buses, const tbf_mix_out* out, void* stream);
/* test hook: the host restatement of the whole definition on host arrays, from the header the
 * kernel is built from (csrc/tbf_mix.h) with libm's fmaf: the arguments of tbf_mix_device, all
 * host memory.  Needs no engine and no device.  -22 as above (no alignment is asked for). */
int tbf_debug_mix_ref (uint32_t n_rows, const float* L, const float* R, uint64_t in_stride, uint32_t frames,
                       const uint32_t* counts, const tbf_mix_row* rows, uint32_t n_buses, const tbf_mix_out* out);
/* test hook: how k_mix lays a call of `frames` frames and n_buses buses out: the frames a lane
 * carries (4, 2 or 1: fewer when the call would otherwise fill too few waves), the frames of a
 * workgroup's tile, and the most buses of one launch (a call with more is launched in slices).
 * No layout changes a bit.  Any pointer may be NULL. */
int tbf_debug_mix_grid (uint32_t frames, uint32_t n_buses, uint32_t* frames_per_lane, uint32_t* tile_frames,
                        uint32_t* slice_buses);
/* k_mix's own time, as tbf_debug_cabinet_time */
int tbf_debug_mix_time (tbf_engine* e, int32_t enable, double* ms, uint64_t* launches);

/* ---- Bus limiter: look-ahead peak limiting of planes, on the device ----
 * A stage behind any two float32 device planes: the buses of tbf_mix_device in front of
 * tbf_pcm_convert_device, or an instance's own L / R.  A feed-forward peak limiter with
 * look-ahead, hold and a linear release.  Like the cabinet, the rate converter, the PCM stage and
 * the mixdown it is specified here, not restated from the reference, which has no limiter
 * (DESIGN.md section 7), and it is defined to the bit, so a limited mix is as reproducible at
 * every cut into calls as the planes behind it.
 * Parameters per limiter, fixed at creation: the ceiling c (float32, finite, 0 < c), ahead = A (a
 * power of two, 2 <= A <= TBF_LIMIT_MAX_AHEAD), hold = H (0 <= H <= TBF_LIMIT_MAX_HOLD).
 * Derived: W = A + H, the latency D = A - 1 frames, the history Hn = A + W - 2 frames per row and
 * channel.
 * For a row with input frames xL[n], xR[n], n counted from the row's first frame since creation
 * or reset, all frames at n < 0 being +0.0f:
 *     p[n]  = 0;  if (fabsf (xL[n]) > p) p = fabsf (xL[n]);  if (fabsf (xR[n]) > p) p = fabsf (xR[n])
 *                                                          (a NaN sample is skipped)
 *     t[n]  = p[n] > c ? c / p[n] : 1.0f                    one correctly rounded float32 division
 *     m[n]  = min (t[n-W+1], ..., t[n])                     exact, any order
 *     acc   = +0.0f;  for j = n-A+1 .. n ascending: acc = acc + m[j]       one float32 add per line
 *     g[n]  = acc * (1.0f / A)                              exact: A is a power of two
 *     yL[n] = g[n] * xL[n-D];  if (yL > c) yL = c;  if (yL < -c) yL = -c;  likewise yR  (NaN stays NaN)
 * Denormals are kept.  NaN and Inf are literal: an Inf gives t = 0 and 0 * Inf = NaN.  The order
 * of the sum is part of the definition: the kernel computes m in any order it likes, but it never
 * re-associates the sum and keeps no running sum.  Because A is a power of two, a row that never
 * exceeds c has g == 1.0f exactly and comes out as its own bits, D frames late, -0.0f and
 * subnormals unchanged.  Every m[j] of the sum covers t[n-D], so g[n] <= t[n-D] up to rounding,
 * and the final clamp makes |y| <= c unconditional.  After a peak the gain stays down for H frames
 * and returns to 1 linearly over A.
 * State: per row and channel the last Hn input frames, zero at creation and at reset.  It belongs
 * to the limiter object, not to an instance: rows are whatever the caller feeds (buses, instances,
 * resampled rows); tbf_instances_* do not know the limiter and tbf_debug_device_bytes does not
 * count its memory.  Row r of a call consumes counts[r] <= frames frames and yields as many;
 * with counts[r] == 0 its state is unchanged.  Nothing depends on how a row's frames are cut into
 * calls.
 * Meters, optional, one per row, overwritten by each call, exact: min_gain = the least g over the
 * row's frames of this call (1.0f for an empty row), reduced = the frames with g < 1.0f, clamped =
 * the samples the final clamp replaced, L and R counted separately. */
#define TBF_LIMIT_MAX_AHEAD 512u
#define TBF_LIMIT_MAX_HOLD 4096u
typedef struct tbf_limiter tbf_limiter;
typedef struct tbf_limiter_config {
	float    ceiling; /* c */
	uint32_t ahead;   /* A */
	uint32_t hold;    /* H */
} tbf_limiter_config;
typedef struct tbf_limit_meter {
	float    min_gain;
	uint32_t reduced, clamped;
} tbf_limit_meter;
typedef struct tbf_limit_out {
	float*           L;      /* n_rows rows, row r from r * stride floats: device memory, 4-byte aligned */
	float*           R;
	uint64_t         stride; /* floats between rows, >= frames */
	tbf_limit_meter* meters; /* optional, one per row: device memory */
} tbf_limit_out;
/* A limiter of n_rows rows on e's device; e owns it: tbf_engine_destroy releases the ones still
 * alive.  -22: a NULL pointer, a ceiling that is not finite or not positive, ahead no power of two
 * or out of range, hold out of range, n_rows == 0.  A host-only engine validates, then returns
 * -19.  -12 when the device cannot hold the state (16 B x Hn per row). */
int tbf_limiter_create (tbf_engine* e, uint32_t n_rows, const tbf_limiter_config* cfg, tbf_limiter** out);
int tbf_limiter_destroy (tbf_limiter* lim);
/* The rows `rows` (host memory, n of them; NULL: all rows, n ignored) start anew, ordered on
 * `stream` (NULL: the engine's own).  -22: a row index >= n_rows. */
int tbf_limiter_reset (tbf_limiter* lim, uint32_t n, const uint32_t* rows, void* stream);
/* D, the frames by which the output trails the input */
int tbf_limiter_latency (const tbf_limiter* lim, uint32_t* frames);
/* One call: the limiter's n_rows rows of d_L / d_R (device memory, row r at r * in_stride floats;
 * any 4-byte-aligned pointers and odd strides, as tbf_render_device delivers them; d_L == d_R is
 * allowed: both outputs are written and are equal) into out->L / out->R on `stream` (NULL: the
 * engine's own), ordered as tbf_render_device: the planes must be complete where `stream` reaches
 * the call, the outputs, meters and state are complete when it has passed it.  Row r takes
 * counts[r] frames (counts: host memory, uploaded before the call returns), or `frames` when
 * counts is NULL.  Nothing outside [0, counts[r]) of an output row is written, and nothing of the
 * meters beyond n_rows.  Calls on one limiter are the caller's to order.
 * -22, with a tbf_last_error that names the argument: a NULL pointer, a stride smaller than the
 * row, a misaligned device pointer, counts[r] > frames, any overlap among the input, the two
 * outputs and the meters (each taken as one range from its first row's first frame to its last
 * row's last; in-place use is refused, because a tile reads its neighbours' input).  Validation
 * comes first: a refused call writes nothing and moves no state. */
int tbf_limit_device (tbf_limiter* lim, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames,
                      const uint32_t* counts, const tbf_limit_out* out, void* stream);
/* test hook: the host restatement of the definition on one row, from the header the kernel is
 * built from (csrc/tbf_limit.h): n frames of L / R (L == R allowed) behind the history histL /
 * histR (Hn floats each, oldest first, read and then replaced by the row's next history) into
 * outL / outR and (optional) one meter.  Needs no engine and no device.  -22 as above. */
int tbf_debug_limit_ref (const tbf_limiter_config* cfg, const float* L, const float* R, uint64_t n, float* histL, float* histR,
                         float* outL, float* outR, tbf_limit_meter* meter);
/* test hook: how k_limit lays a configuration out: the frames a lane carries at a time, the frames
 * of a workgroup's tile (a function of the configuration alone), the history Hn and the
 * workgroup's LDS bytes.  No layout changes a bit.  Any out pointer may be NULL.  -22 as
 * tbf_limiter_create. */
int tbf_debug_limit_grid (const tbf_limiter_config* cfg, uint32_t* frames_per_lane, uint32_t* tile_frames, uint32_t* history,
                          uint32_t* lds_bytes);
/* k_limit's own time (with its meter preset, when a call has meters), as tbf_debug_cabinet_time:
 * one launch set per call that took frames */
int tbf_debug_limit_time (tbf_limiter* lim, int32_t enable, double* ms, uint64_t* launches);

/* -- Bus limiter, addition: a true-peak detector --
 * A limiter may be created with a detector that sees the oversampled waveform: oversample F in
 * {2, 4}, the interpolator and its phases those of the true-peak meter below (tpeak_phase: {0, 1, 2, 3}
 * for F = 4, {0, 2} for F = 2; a caller picks F from its rate as there: 4 below 96 kHz, 2 below
 * 192 kHz; at or above 192 kHz the plain limiter is the one to use).  Let E = 6.  For a row, all
 * frames before its first being +0.0f:
 *     yc[n][p] = the meter's chain: acc = +0.0f; for j = 0 .. 11 ascending: acc = fmaf (h[p][j], xc[n-j], acc)
 *                                                                                  c in {L, R}
 *     p[n]  = 0;  for v in { xL[n-E], xR[n-E], yL[n][p], yR[n][p] for every phase p used }:
 *                     if (fabsf (v) > p[n]) p[n] = fabsf (v)      (a NaN is skipped; exact in any order)
 *     t[n], m[n], g[n]   exactly as above: c / p[n] or 1.0f, the minimum over W = A + H, the
 *                        ascending chain of A adds, * 1/A
 *     yL[n] = g[n] * xL[n-D-E], clamped to [-c, c] as above; likewise yR       D = A - 1
 * Why E = 6: the interpolated values of frame n lie between the input frames n-6 and n-5, where the
 * table's main taps are (j = 6 for phases 0 and 1, j = 5 for phases 2 and 3).  Pairing them with
 * the sample E = 6 frames back makes p[n] the peak of one stretch of the oversampled waveform, from
 * sample n-6 up to but not including sample n-5.  The audio is delayed by the same E, so g[n] <=
 * t[n-D] (up to rounding, as above) still covers the sample it multiplies.
 * Consequences:
 *   - The latency is D + E = A + 5 frames (tbf_limiter_latency reports it).
 *   - The history is Hn_tp = 2 A + H + 9 frames per row and channel: g[n] reaches t[n-Hn] with
 *     Hn = 2 A + H - 2, and t[f] reaches x[f-11].
 *   - |y| <= c stays unconditional, through the clamp.
 *   - A row whose p never exceeds c has g == 1.0f and comes out as its own bits, A + 5 frames late,
 *     -0.0f and subnormals unchanged.
 *   - A row whose samples stay under c but whose interpolated values do not is reduced.
 *   - A NaN sample is skipped, and so is every interpolated value whose window it touches (the
 *     chain's result is a NaN, which compares false): for those twelve frames p falls back to the
 *     sample peaks.  An Inf is literal: a sample Inf gives t = 0; in a chain it gives Inf or
 *     (Inf - Inf) a NaN, which is skipped.
 *   - An inter-sample peak between x[k] and x[k+1] belongs to p[k+6].  The gain of x[k] covers it
 *     for any H (g[k+D+E] <= t[k+6]); the gain of x[k+1], g[k+1+D+E], sums m[k+7 .. k+A+6], whose
 *     windows reach back to t[k+6] only when H >= 1.  So both neighbours of an inter-sample peak
 *     are turned down by its target only with H >= 1; with H = 0 the later one may already be one
 *     step of the release up.
 *   - The true peak of the output is not bounded in general: twelve samples with twelve gains enter
 *     one interpolated value.  It is bounded where the gain is constant: there y = g x up to one
 *     rounding a sample, the chains are linear, and the output's interpolated values are g times
 *     the input's up to the products' and the chains' roundings, within c (1 + 2^-18) for the
 *     annex's table (sum |h| < 2.03).
 * The meters are the same three and are exact.  The state is raw input only, in two sides as
 * above; it belongs to the limiter object and is not saved.  tbf_limit_device, tbf_limiter_reset,
 * tbf_limiter_destroy and tbf_debug_limit_time serve both kinds. */
typedef struct tbf_limiter_detect {
	uint32_t oversample, reserved; /* F in {2, 4}; 0 */
} tbf_limiter_detect;
/* As tbf_limiter_create, with the detector above.  -22 in addition: det NULL, an oversample that is
 * neither 2 nor 4, reserved != 0.  A host-only engine validates, then returns -19.  -12 when the
 * device cannot hold the state (16 B x Hn_tp per row). */
int tbf_limiter_create_tp (tbf_engine* e, uint32_t n_rows, const tbf_limiter_config* cfg, const tbf_limiter_detect* det,
                           tbf_limiter** out);
/* test hook: the host restatement of the definition with the detector on one row, from the headers
 * the kernel is built from (limit_target, limit_out and limit_tp_peak of csrc/tbf_limit.h, tpeak_y
 * of csrc/tbf_tpeak.h): as tbf_debug_limit_ref, the histories Hn_tp floats each, oldest first, read
 * and then replaced. */
int tbf_debug_limit_tp_ref (const tbf_limiter_config* cfg, const tbf_limiter_detect* det, const float* L, const float* R, uint64_t n,
                            float* histL, float* histR, float* outL, float* outR, tbf_limit_meter* meter);
/* test hook: how k_limit_tp lays a configuration out, as tbf_debug_limit_grid: the history is
 * Hn_tp and the LDS bytes include the raw samples of one pass */
int tbf_debug_limit_tp_grid (const tbf_limiter_config* cfg, const tbf_limiter_detect* det, uint32_t* frames_per_lane,
                             uint32_t* tile_frames, uint32_t* history, uint32_t* lds_bytes);

/* ---- Loudness meter: BS.1770 integrated loudness of planes, on the device ----
 * A stage beside any two float32 device planes: it reads them and writes only its own memory.
 * ITU-R BS.1770-4 integrated loudness with EBU R128 gating, for a stereo pair with both channel
 * weights 1.0.  Like the mixdown and the limiter it is specified here, not restated from the
 * reference, which has no meter, and it is defined to the bit up to the hop
 * energies.  With a loudness per row, normalisation needs no stage of its own: tbf_mix_device with
 * one bus per row and ll = rr = gain applies a per-row gain in front of the limiter.
 * Parameters per meter, fixed at creation: rate_hz, an integer in [8000, 192000] and a multiple of
 * 10; max_hops >= 1, the most 100 ms hops a row can hold between resets.  Derived: Hp = rate_hz / 10
 * frames per hop.
 * Coefficients: seven doubles, computed on the host once per meter in double with libm; the kernel
 * receives them and never derives them.
 *     shelf:  f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196
 *             K = tan (pi*f0/rate); Vh = pow (10, G/20); Vb = pow (Vh, 0.4996667741545416); a0 = 1 + K/Q + K*K
 *             b0 = (Vh + Vb*K/Q + K*K)/a0;  b1 = 2*(K*K - Vh)/a0;  b2 = (Vh - Vb*K/Q + K*K)/a0
 *             a1 = 2*(K*K - 1)/a0;          a2 = (1 - K/Q + K*K)/a0
 *     high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773, K = tan (pi*f0/rate), a0 = 1 + K/Q + K*K
 *             numerator 1, -2, 1 (literal);  c1 = 2*(K*K - 1)/a0;  c2 = (1 - K/Q + K*K)/a0
 * (at 48000 these are the standard's printed table to its last digit.)
 * Per row, per channel, per input frame, x = (double) sample; every *, + and - is one IEEE double
 * operation, with no contraction, no fma and no flushing:
 *     y  = b0*x + s1;   s1 = (b1*x + s2) - a1*y;    s2 = b2*x - a2*y
 *     w  = y + t1;      t1 = (-2.0*y + t2) - c1*w;  t2 = y - c2*w
 *     acc = acc + w*w;  k = k + 1
 *     if (k == Hp) { E[row][hop][channel] = acc; acc = +0.0; k = 0; hop = hop + 1 }
 * All state is zero at creation and at reset.  NaN and Inf are literal: a NaN poisons its row until
 * the row is reset, and it touches no other row.  The order is part of the definition: a channel's
 * frames form one serial chain; the kernel parallelises over rows and channels, never over a row's
 * time, and keeps no block-wise transition matrices and no tree sums.  So a row's hop energies are
 * the same bits however its frames are cut into calls.  d_L == d_R is allowed: such a row is
 * measured as a pair of equal channels.
 * Results, computed on the host in double by tbf_loudness_read from the row's N complete hops (an
 * unfinished hop does not count):
 *     u_h = EL_h + ER_h
 *     z_j = (((u_j + u_{j+1}) + u_{j+2}) + u_{j+3}) / (4*Hp), j = 0 .. N-4          block energy
 *     l_j = -0.691 + 10*log10 (z_j)                                                block loudness
 *     absolute gate: l_j > -70;   relative gate: G = -0.691 + 10*log10 (mean z over the absolutely
 *     gated blocks) - 10
 *     integrated = -0.691 + 10*log10 (mean z over the blocks with l_j > -70 and l_j > G), the means
 *     ascending serial sums
 *     momentary_max = max l_j;  short_term_max the same over 30-hop (3 s) windows of u, once N >= 30
 * A quantity with no block to take it from is -HUGE_VAL.  hops = N, blocks = the 400 ms blocks,
 * gated = the blocks behind `integrated`.  These go through libm's log10 and are compared to a
 * tolerance; the hop energies are compared in bits.
 * State: 16 B x max_hops + 96 B per row.  It belongs to the meter object, not to an instance:
 * tbf_instances_* do not know it, tbf_debug_device_bytes does not count it, and it is not saved.
 * Loudness range (EBU Tech 3342), computed on the host in double by tbf_loudness_range from the
 * same N complete hops, u_h as above:
 *     z_j = (serial ascending sum of u_j .. u_{j+29}) / (30*Hp), j = 0 .. N-30      short-term windows
 *     l_j = -0.691 + 10*log10 (z_j)
 *     absolute gate: l_j > -70;   relative gate: l_j > (-0.691 + 10*log10 (mean z over the absolutely
 *     gated windows, an ascending serial sum)) - 20
 *     s[0 .. n-1] the surviving l sorted ascending
 *     LRA = s[floor ((n-1)*0.95 + 0.5)] - s[floor ((n-1)*0.10 + 0.5)];  windows = n;  LRA = 0.0 when n = 0
 * Left out: channel counts other than the pair, saving a meter.  (True peak is the next section.) */
typedef struct tbf_loudness tbf_loudness;
typedef struct tbf_loudness_config {
	uint32_t rate_hz, max_hops;
} tbf_loudness_config;
typedef struct tbf_loudness_result {
	double   integrated, momentary_max, short_term_max; /* LUFS, or -HUGE_VAL */
	uint32_t hops, blocks, gated, reserved;
} tbf_loudness_result;
/* A meter of n_rows rows on e's device; e owns it: tbf_engine_destroy releases the ones still
 * alive.  -22: a NULL pointer, a rate_hz out of range or no multiple of 10, max_hops == 0,
 * n_rows == 0.  A host-only engine validates, then returns -19.  -12 when the device cannot hold
 * the state. */
int tbf_loudness_create (tbf_engine* e, uint32_t n_rows, const tbf_loudness_config* cfg, tbf_loudness** out);
int tbf_loudness_destroy (tbf_loudness* lm);
/* The rows `rows` (host memory, n of them; NULL: all rows, n ignored) start anew, ordered on
 * `stream` (NULL: the engine's own).  -22: a row index >= n_rows. */
int tbf_loudness_reset (tbf_loudness* lm, uint32_t n, const uint32_t* rows, void* stream);
/* One call: the meter's n_rows rows of d_L / d_R (device memory, row r at r * in_stride floats; any
 * 4-byte-aligned pointers and odd strides; d_L == d_R allowed) on `stream` (NULL: the engine's
 * own), ordered as tbf_render_device.  The planes are only read.  Row r takes counts[r] <= frames
 * frames (counts: host memory, uploaded before the call returns), or `frames` when counts is NULL;
 * a row with count 0 keeps its state.  Calls on one meter are the caller's to order.
 * -22, with a tbf_last_error that names the argument: a NULL pointer, in_stride < frames, a
 * misaligned pointer, counts[r] > frames.  -28 when some row would complete more than max_hops
 * hops (the host knows every row's position).  Validation comes first: a refused call moves no
 * state. */
int tbf_loudness_device (tbf_loudness* lm, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames,
                         const uint32_t* counts, void* stream);
/* The results of the rows `rows` (n of them; NULL: all rows in order, n ignored) into out.  Waits
 * for the meter's last call on its stream.  -22: a NULL pointer, a row index >= n_rows. */
int tbf_loudness_read (tbf_loudness* lm, uint32_t n, const uint32_t* rows, tbf_loudness_result* out);
/* The energies of a row's complete hops as EL, ER pairs into e (room for cap_hops pairs) and
 * their number into n_hops; waits as tbf_loudness_read.  -28 when cap_hops is too small, with
 * n_hops set and nothing else written. */
int tbf_loudness_hops (tbf_loudness* lm, uint32_t row, double* e, uint32_t cap_hops, uint32_t* n_hops);
/* test hook: the seven coefficients b0, b1, b2, a1, a2, c1, c2 of a rate.  -22 as tbf_loudness_create. */
int tbf_debug_loudness_coeffs (uint32_t rate_hz, double* c7);
/* test hook: the host restatement of the definition on one row, from the header the kernel is
 * built from (csrc/tbf_loud.h): n frames of L / R (L == R allowed) behind `state` = {s1, s2, t1, t2,
 * acc, k} of L followed by the same of R (12 doubles, read and then replaced); the energies of the
 * hops completed by these frames as EL, ER pairs into e and their number into n_hops.  Needs no
 * engine and no device.  -22 as above, and for a state whose k is no integer in [0, Hp); -28 when
 * cap_hops is too small, with nothing written. */
int tbf_debug_loudness_ref (const tbf_loudness_config* cfg, const float* L, const float* R, uint64_t n, double* state,
                            double* e, uint32_t cap_hops, uint32_t* n_hops);
/* test hook: the gating alone, on n_hops EL, ER pairs in host memory; tbf_loudness_read calls the
 * same code */
int tbf_debug_loudness_result (uint32_t rate_hz, const double* e, uint32_t n_hops, tbf_loudness_result* out);
/* test hook: how k_loud lays a meter of n_rows rows out: the rows of a workgroup, the frames of a
 * row staged in LDS at a time, and the workgroup's LDS bytes.  No layout changes a bit.  Any out
 * pointer may be NULL. */
int tbf_debug_loudness_grid (uint32_t n_rows, uint32_t* rows_per_group, uint32_t* tile_frames, uint32_t* lds_bytes);
/* k_loud's own time, as tbf_debug_limit_time: one launch set per call that took frames */
int tbf_debug_loudness_time (tbf_loudness* lm, int32_t enable, double* ms, uint64_t* launches);
/* The loudness range in LU of the rows `rows` (n of them; NULL: all rows in order, n ignored) into
 * lra, and the windows behind each into windows (may be NULL).  Waits as tbf_loudness_read.  -22: a
 * NULL pointer, a row index >= n_rows. */
int tbf_loudness_range (tbf_loudness* lm, uint32_t n, const uint32_t* rows, double* lra, uint32_t* windows);
/* test hook: the range arithmetic alone, on n_hops EL, ER pairs in host memory; tbf_loudness_range
 * calls the same code.  windows may be NULL. */
int tbf_debug_loudness_range (uint32_t rate_hz, const double* e, uint32_t n_hops, double* lra, uint32_t* windows);

/* ---- True-peak meter: oversampled inter-sample peaks of planes, on the device ----
 * A stage beside any two float32 device planes: it reads them and writes only its own memory.  The
 * limiter bounds the samples and k_pcm counts the samples that clip; this stage measures what lies
 * between them, as ITU-R BS.1770-4 Annex 2 does.  Like the mixdown, the limiter and the loudness
 * meter it is specified here, not restated from the reference, which has no meter (DESIGN.md
 * section 7), and it is defined to the bit.
 * Table: 4 phases x 12 taps, h[p][j] = k[p][j] / 8192, every coefficient exact in float32:
 *     k[0] = {   14,  90, -161, 272,  -487, 1125, 7964,  -838, 390, -218, 122,  -68 }
 *     k[1] = { -239, 240, -424, 730, -1364, 3810, 6388, -1641, 832, -477, 271, -155 }
 *     k[2] = k[1] reversed,   k[3] = k[0] reversed
 * (the annex's printed table: phase 0 is 0.0017089843750, 0.0109863281250, -0.0196533203125, ...).
 * Parameter per meter, fixed at creation: oversample F in {1, 2, 4}.  The phases used are {0, 1, 2, 3}
 * for F = 4, {0, 2} for F = 2 and none for F = 1.  (A caller picks F from its rate: 4 below 96 kHz, 2
 * below 192 kHz, otherwise 1.)
 * Per row, per channel, per input frame n: x[n] is the float32 sample and x[m] for m before the
 * row's first frame since creation or reset is +0.0f.  For every phase p used:
 *     acc = +0.0f;  for j = 0 .. 11 ascending:  acc = fmaf (h[p][j], x[n - j], acc);   y[n][p] = acc
 *     inter_peak  = umax (inter_peak,  bits (y[n][p]) & 0x7fffffff)
 *     sample_peak = umax (sample_peak, bits (x[n])    & 0x7fffffff)
 * umax is the unsigned 32-bit maximum of the bit patterns of the magnitudes: on finite values the
 * float maximum; Inf above every finite value and a NaN above Inf, so a NaN poisons its row and
 * channel until reset and touches no other row; and, an integer maximum, exact in any order.  The tap
 * order of each y is part of the definition: one float32 fmaf per tap, no contraction beyond it, no
 * flushing.  The order in which the y are compared is not, which leaves the kernel free to be
 * parallel over time.  A row's peaks are therefore the same bits however its frames are cut into
 * calls.  A NaN's payload is not defined: a NaN result is compared as "is NaN", all else in bits.
 * d_L == d_R is allowed: such a row is measured as a pair of equal channels.
 * Read-out per row: sample_peak[2] and inter_peak[2] as floats (L, R), frames taken since reset, and
 *     dbtp = 20*log10 (the largest of the four), in double on the host; -HUGE_VAL when that is 0,
 *     NaN when it is a NaN.
 * The samples are part of the maximum, so dbtp is never below the sample peak and F = 1 has a meaning.
 * State: 200 B per row (two sides of 2 x 11 floats of history, four words of peaks, one record of
 * the call).  It belongs to the meter object, not to an instance: tbf_instances_* do not know it,
 * tbf_debug_device_bytes does not count it, and it is not saved.
 * Left out: a per-hop series, surround weights, saving a meter.  (Detection inside the limiter is
 * tbf_limiter_create_tp, in the limiter's section.) */
typedef struct tbf_true_peak tbf_true_peak;
typedef struct tbf_true_peak_config {
	uint32_t oversample, reserved;
} tbf_true_peak_config;
typedef struct tbf_true_peak_result {
	float    sample_peak[2], inter_peak[2]; /* L, R */
	uint64_t frames;
	double   dbtp; /* or -HUGE_VAL, or NaN */
} tbf_true_peak_result;
/* A meter of n_rows rows on e's device; e owns it: tbf_engine_destroy releases the ones still
 * alive.  -22: a NULL pointer, an oversample not in {1, 2, 4}, n_rows == 0.  A host-only engine
 * validates, then returns -19.  -12 when the device cannot hold the state. */
int tbf_true_peak_create (tbf_engine* e, uint32_t n_rows, const tbf_true_peak_config* cfg, tbf_true_peak** out);
int tbf_true_peak_destroy (tbf_true_peak* tp);
/* The rows `rows` (host memory, n of them; NULL: all rows, n ignored) start anew, ordered on
 * `stream` (NULL: the engine's own).  -22: a row index >= n_rows. */
int tbf_true_peak_reset (tbf_true_peak* tp, uint32_t n, const uint32_t* rows, void* stream);
/* One call: the meter's n_rows rows of d_L / d_R (device memory, row r at r * in_stride floats; any
 * 4-byte-aligned pointers and odd strides; d_L == d_R allowed) on `stream` (NULL: the engine's
 * own), ordered as tbf_render_device.  The planes are only read.  Row r takes counts[r] <= frames
 * frames (counts: host memory, uploaded before the call returns), or `frames` when counts is NULL;
 * a row with count 0 keeps its state.  Calls on one meter are the caller's to order.
 * -22, with a tbf_last_error that names the argument: a NULL pointer, in_stride < frames, a
 * misaligned pointer, counts[r] > frames, more than 2^31 - 1 tiles of 1024 frames over all rows.
 * Validation comes first: a refused call moves no state. */
int tbf_true_peak_device (tbf_true_peak* tp, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames,
                          const uint32_t* counts, void* stream);
/* The results of the rows `rows` (n of them; NULL: all rows in order, n ignored) into out.  Waits
 * for the meter's last call on its stream.  -22: a NULL pointer, a row index >= n_rows. */
int tbf_true_peak_read (tbf_true_peak* tp, uint32_t n, const uint32_t* rows, tbf_true_peak_result* out);
/* test hook: the table h[p][j] as 48 floats, phase-major */
int tbf_debug_true_peak_table (float* h48);
/* test hook: the host restatement of the definition on one row, from the header the kernel is
 * built from (csrc/tbf_tpeak.h): n frames of L / R (L == R allowed) behind hist22 = L's last 11
 * frames, oldest first, followed by R's (read and then replaced by the last 11 of history ||
 * frames) into peaks4 = the bit patterns {sample L, sample R, inter L, inter R} (read and then
 * replaced).  y NULL, or room for every y[n][p]: L's n * P floats, frame-major, followed by R's,
 * P = 4, 2 or 0 phases for oversample 4, 2, 1.  Needs no engine and no device. */
int tbf_debug_true_peak_ref (const tbf_true_peak_config* cfg, const float* L, const float* R, uint64_t n, float* hist22,
                             uint32_t* peaks4, float* y);
/* test hook: the read-out's dbtp of four peak words */
int tbf_debug_true_peak_dbtp (const uint32_t* peaks4, double* dbtp);
/* test hook: how k_tpeak lays a call of `frames` frames on n_rows rows out: the frames of a row a
 * workgroup takes (the tile), the consecutive frames of a lane, the workgroups of the launch and a
 * workgroup's LDS bytes.  No layout changes a bit.  Any out pointer may be NULL. */
int tbf_debug_true_peak_grid (uint32_t n_rows, uint32_t frames, uint32_t* tile_frames, uint32_t* frames_per_lane, uint64_t* groups,
                              uint32_t* lds_bytes);
/* k_tpeak's own time, as tbf_debug_loudness_time: one launch per call that took frames */
int tbf_debug_true_peak_time (tbf_true_peak* tp, int32_t enable, double* ms, uint64_t* launches);

/* ---- Bus equaliser: parametric bands on planes, band-pipelined on the device ----
 * A stage between two pairs of float32 device planes: tone shaping of a bus, between the mixdown and
 * the limiter: a rumble high-pass, a shelf, a notch or a bell per row.  Like the mixdown, the
 * limiter and the meters it is specified here, not restated from the reference, which equalises
 * nothing but the whirl's own filters, and it is defined to the bit.
 * Parameters per equaliser, fixed at creation: rate_hz, an integer in [8000, 192000]; max_bands in
 * 1 .. 8 (TBF_EQ_MAX_BANDS); n_rows >= 1.  Derived: P, the smallest of 1, 2, 4, 8 that is >=
 * max_bands, the lanes k_eq gives a row and channel; no P changes a bit.
 * Bands: a row has nb <= max_bands bands {type, hz, q, gain_db}, none at creation.  The types are
 * the reference designer's (src/eqcomp.cpp): 0 LPF, 1 HPF, 2 BPF0 (peak gain Q), 3 BPF1 (0 dB peak),
 * 4 notch, 5 APF, 6 PEQ, 7 low shelf, 8 high shelf.  Accepted: 0.1 < q < 6 and 0.0002 < hz / rate_hz <
 * 0.4998, which is the guard of the reference's setIIRFilter, and |gain_db| <= 24.  Anything else,
 * a NaN included, is refused with -22 and a tbf_last_error that names the row and the band; nothing
 * is silently kept.
 * Coefficients: five doubles {b0, b1, b2, a1, a2} per band, computed on the host in double with
 * libm by the RBJ designer that the whirl's filters use (eqCompute, csrc/tbf_eq.h) and normalised by
 * a0 as it does; the kernel receives them and never derives them.  With A = pow (10, gain_db / 40),
 * w = 2*pi*hz / rate_hz, alpha = sin (w) / (2*q), beta = sqrt (A) / q, each of b0, b1, b2, a1, a2 is
 * the listed value divided by a0:
 *     LPF    b (1-cos w)/2, 1-cos w, (1-cos w)/2              a 1+alpha, -2 cos w, 1-alpha
 *     HPF    b (1+cos w)/2, -(1+cos w), (1+cos w)/2           a as LPF
 *     BPF0   b sin w/2, 0, -sin w/2                           a as LPF
 *     BPF1   b alpha, 0, -alpha                               a as LPF
 *     notch  b 1, -2 cos w, 1                                 a as LPF
 *     APF    b 1-alpha, -2 cos w, 1+alpha                     a as LPF
 *     PEQ    b 1+alpha*A, -2 cos w, 1-alpha*A                 a 1+alpha/A, -2 cos w, 1-alpha/A
 *     low    b A((A+1)-(A-1)cos w+beta sin w), 2A((A-1)-(A+1)cos w), A((A+1)-(A-1)cos w-beta sin w)
 *            a (A+1)+(A-1)cos w+beta sin w, -2((A-1)+(A+1)cos w), (A+1)+(A-1)cos w-beta sin w
 *     high   b A((A+1)+(A-1)cos w+beta sin w), -2A((A-1)+(A+1)cos w), A((A+1)+(A-1)cos w-beta sin w)
 *            a (A+1)-(A-1)cos w+beta sin w, 2((A-1)-(A+1)cos w), (A+1)-(A-1)cos w-beta sin w
 * Per row, per channel, per frame, v = (double) sample, then for each band b = 0 .. nb - 1 in order,
 * in transposed direct form II, every *, + and - one IEEE double operation, with no contraction, no
 * fma and no flushing:
 *     y = b0*v + s1;   s1 = (b1*v + s2) - a1*y;   s2 = b2*v - a2*y;   v = y
 * and the output is (float) v, one round-to-nearest.  A row with nb = 0 passes through: every
 * non-NaN input comes out as its own bits, and a NaN stays a NaN.  NaN and Inf are literal: a
 * poisoned row stays poisoned until it is reset, and it touches no other row.  Which NaN comes out
 * (its sign and payload) is not part of the definition: hosts and the device differ there.
 * State: two doubles per row, channel and band (32 B x max_bands per row), zero at creation and at
 * reset.  It belongs to the equaliser object, not to an instance: tbf_instances_* do not know it,
 * tbf_debug_device_bytes does not count it, and it is not saved.
 * The order is part of the definition.  A band's frames form one serial chain, and band b of frame
 * n needs only band b - 1 of frame n and its own state of frame n - 1: the kernel runs a row and
 * channel's bands as a pipeline over adjacent lanes, one frame apart, and drains it before a call
 * ends.  It parallelises over rows, channels and bands, never over a row's time, and keeps no
 * transition matrices.  So a row's output has the same bits however its frames are cut into calls,
 * whatever P is, and whatever rows stand beside it.
 * Left out: parameter ramps (tbf_eq_set switches a row's coefficients between two calls, as the
 * reference's setIIRFilter does between two blocks), saving an equaliser's state, linear-phase
 * filters, and band lists per channel. */
#define TBF_EQ_MAX_BANDS 8u
#define TBF_EQ_LPF 0
#define TBF_EQ_HPF 1
#define TBF_EQ_BPF0 2
#define TBF_EQ_BPF1 3
#define TBF_EQ_NOTCH 4
#define TBF_EQ_APF 5
#define TBF_EQ_PEQ 6
#define TBF_EQ_LOW 7
#define TBF_EQ_HIGH 8
typedef struct tbf_eq tbf_eq;
typedef struct tbf_eq_config {
	uint32_t rate_hz, max_bands;
} tbf_eq_config;
typedef struct tbf_eq_band {
	int32_t type, reserved; /* TBF_EQ_*; reserved is ignored */
	double  hz, q, gain_db; /* gain_db matters to PEQ and the shelves only, and is checked for all */
} tbf_eq_band;
/* An equaliser of n_rows rows, none with a band, on e's device; e owns it: tbf_engine_destroy
 * releases the ones still alive.  -22: a NULL pointer, a rate_hz or max_bands out of range,
 * n_rows == 0.  A host-only engine validates, then returns -19.  -12 when the device cannot hold
 * the state. */
int tbf_eq_create (tbf_engine* e, uint32_t n_rows, const tbf_eq_config* cfg, tbf_eq** out);
int tbf_eq_destroy (tbf_eq* eq);
/* The state of the rows `rows` (host memory, n of them; NULL: all rows, n ignored) is zero again,
 * ordered on `stream` (NULL: the engine's own); their bands stay.  -22: a row index >= n_rows. */
int tbf_eq_reset (tbf_eq* eq, uint32_t n, const uint32_t* rows, void* stream);
/* New band lists for the rows `rows` (n of them; NULL: all rows in order, n ignored): row k of the
 * list takes n_bands[k] <= max_bands bands, which stand packed in `bands`, row k's behind those of
 * the rows before it (bands may be NULL when every n_bands[k] is 0).  Ordered on `stream` (NULL: the
 * engine's own) as tbf_eq_reset is: it takes effect from the next tbf_eq_device on, and the state is
 * kept, as the reference's setIIRFilter keeps its filter's z.  The upload is staged in the
 * equaliser's own tables, and the call waits for `stream` before it returns, so the staging outlives
 * the copy and the caller's arrays are free at once.  Every band of every row is checked before
 * anything changes: -22 (see above) leaves every row as it was. */
int tbf_eq_set (tbf_eq* eq, uint32_t n, const uint32_t* rows, const tbf_eq_band* bands, const uint32_t* n_bands, void* stream);
/* The read-back: a row's bands in use into nb and their coefficients, five doubles {b0, b1, b2, a1,
 * a2} per band, into coeffs (room for `cap` bands).  From the host's tables: no wait.  -28 when cap
 * is too small, with nb set and nothing else written. */
int tbf_eq_bands (const tbf_eq* eq, uint32_t row, double* coeffs, uint32_t cap, uint32_t* nb);
/* One call: the equaliser's n_rows rows of d_L / d_R (device memory, row r at r * in_stride floats;
 * any 4-byte-aligned pointers and odd strides; d_L == d_R allowed: mono in, two equal planes out)
 * into d_outL / d_outR (row r at r * out_stride floats) on `stream` (NULL: the engine's own),
 * ordered as tbf_render_device.  Row r takes counts[r] <= frames frames (counts: host memory,
 * uploaded before the call returns, for which the call waits for `stream`; NULL: `frames` each, and
 * no wait); a row with count 0 keeps its state.  Output rows are written in [0, count) and left
 * alone behind it; the inputs are only read.  Calls on one equaliser are the caller's to order.
 * -22, with a tbf_last_error that names the argument: a NULL pointer, in_stride or out_stride <
 * frames, a misaligned pointer, counts[r] > frames, an output that overlaps an input or the other
 * output.  Validation comes first: a refused call moves no state. */
int tbf_eq_device (tbf_eq* eq, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames, float* d_outL, float* d_outR,
                   uint64_t out_stride, const uint32_t* counts, void* stream);
/* test hook: the five coefficients of one band at a rate.  Needs no engine.  -22 as tbf_eq_set
 * (the error names row 0 band 0). */
int tbf_debug_eq_coeffs (uint32_t rate_hz, const tbf_eq_band* band, double* c5);
/* test hook: the host restatement of the definition on one row, from the header the kernel is
 * built from (csrc/tbf_eq.h): n frames of L / R (L == R allowed) through nb <= 8 bands with the
 * coefficients coeffs[nb][5], behind `state` = L's {s1, s2} per band followed by R's (4 nb doubles,
 * read and then replaced), into outL / outR.  Needs no engine and no device. */
int tbf_debug_eq_ref (const double* coeffs, uint32_t nb, const float* L, const float* R, uint64_t n, double* state, float* outL,
                      float* outR);
/* test hook: how k_eq lays an equaliser of max_bands out: P, the rows of a wave (32 / P), the frames
 * of a row staged in LDS at a time, and the workgroup's LDS bytes.  No layout changes a bit.  Any
 * out pointer may be NULL.  -22: max_bands out of range. */
int tbf_debug_eq_grid (uint32_t max_bands, uint32_t* lanes, uint32_t* rows_per_wave, uint32_t* tile_frames, uint32_t* lds_bytes);
/* k_eq's own time, as tbf_debug_loudness_time: one launch per call that took frames */
int tbf_debug_eq_time (tbf_eq* eq, int32_t enable, double* ms, uint64_t* launches);

/* ---- Bus compressor: recursive attack and release on planes, on the device ----
 * A stage between two pairs of float32 device planes: the dynamics of a bus, between the equaliser
 * and the limiter: threshold, ratio and knee as a gain curve, attack, release and make-up per row,
 * and an optional key pair for ducking.  Like the mixdown, the equaliser, the limiter and the meters
 * it is specified here, not restated from the reference, which has no dynamics processor (DESIGN.md
 * section 7), and it is defined to the bit.
 * Per compressor, fixed at creation: n_rows >= 1 rows and n_curves gain curves, 1 ..
 * TBF_COMP_MAX_CURVES = 8.  Per row four parameters: curve (default 0), attack, a float32
 * coefficient a (default 0), release, a float32 coefficient r (default 0), and makeup, a float32 m
 * (default 1); and one state float g, 1.0f at creation and at reset.
 * Curve: a curve is data, TBF_COMP_POINTS = 769 float32 gains pt[0 .. 768] on a grid of
 * TBF_COMP_SEG = 32 segments per octave over the 24 octaves from 2^-16 to 2^8: point i is the gain
 * at the level 2^(-16 + i/32) * (1 + (i%32)/32) (i/32 the integer quotient).  Every curve is all
 * 1.0f at creation.  The kernel never derives a curve.  With u the bit pattern of the level p, a
 * float32 >= 0 and never NaN:
 *     i  = (u >> 18) - (111 << 5)
 *     fr = (float) (u & 0x3FFFF) * 2^-18                     exact
 *     t  = fmaf (fr, pt[i+1] - pt[i], pt[i])                 for 0 <= i < 768: one float32
 *                                                            subtraction and one fmaf
 *     t  = pt[0] for p < 2^-16, and t = pt[768] for p >= 2^8, +Inf included.
 * A grid level returns its own point; hard knees are smoothed over one segment.
 * Per frame n of a row, in this order, every operation one float32 operation, denormals kept:
 *     p[n] = limit_peak (kL[n], kR[n])      the limiter's: the larger magnitude, NaN skipped, so p
 *                                           is never NaN; k is the key pair when the call gives
 *                                           one, otherwise the input pair
 *     t[n] = the row's curve at p[n], as above
 *     d    = g[n-1] - t[n];   g[n] = fmaf (d > 0 ? a : r, d, t[n])
 *                                           the attack coefficient applies while the gain must fall
 *     y[n] = (g[n] * m) * x[n]              for each channel: two multiplies in that order; NaN and
 *                                           Inf in x are literal
 * The latency is 0 frames.  Consequences: a row on a flat curve with m = 1 comes out as its own
 * bits (g stays exactly 1.0f, and a NaN stays a NaN); g is always finite and in [0, 1], because the
 * points are, so a NaN in the audio cannot poison the state; and, the recurrence being the only
 * thing that crosses a frame, a row has the same bits however its frames are cut into calls,
 * whatever layout the kernel chose, and whatever rows stand beside it.  Which NaN comes out (its
 * sign and payload) is not part of the definition.
 * Accepted: every point finite and in [0, 1] (-0.0f is not: a gain's bits order as its value); a
 * and r in [0, 1); m finite and in [0,
 * TBF_COMP_MAX_MAKEUP = 256]; curve < n_curves.  Anything else, a NaN included, is refused with -22
 * and a tbf_last_error that names the row or the point; nothing has changed when a call is refused.
 * Designer (host, double, libm): tbf_comp_curve_design (threshold_db T, ratio R, knee_db W) fills the
 * 769 points: with x = 20 log10 (level),
 *     2 (x - T) < -W:    y = x
 *     2 |x - T| <= W:    y = x + (1/R - 1) (x - T + W/2)^2 / (2 W)
 *     otherwise:         y = T + (x - T) / R
 * and gain = min (1, 10^((y - x) / 20)), rounded once to float.  Accepted: -90 <= T <= 0, 1 <= R <=
 * +Inf (1/R = 0: a limiter curve), 0 <= W <= 40.  The designer is held to a tolerance, not to bits.
 * Gates, expanders and any other shape are the caller's own 769 points.
 * State: one float per row.  It belongs to the compressor object, not to an instance:
 * tbf_instances_* do not know it, tbf_debug_device_bytes does not count it, and it is not saved.
 * Left out: look-ahead (the limiter has it), RMS or K-weighted detection, per-channel (unlinked)
 * gain, parameter ramps, saving a compressor's state, and upward gain from the curve (points above
 * 1). */
#define TBF_COMP_MAX_CURVES 8u
#define TBF_COMP_SEG 32u
#define TBF_COMP_POINTS 769u
#define TBF_COMP_MAX_MAKEUP 256.0f
typedef struct tbf_comp tbf_comp;
typedef struct tbf_comp_config {
	uint32_t n_curves;
} tbf_comp_config;
typedef struct tbf_comp_row {
	uint32_t curve;
	float    attack, release, makeup;
} tbf_comp_row;
typedef struct tbf_comp_meter {
	float    min_gain; /* the smallest g[n] of the call's frames of the row; 1.0f when it took none */
	uint32_t frames;   /* the row's frames of the call */
} tbf_comp_meter;
/* A compressor of n_rows rows, every curve flat and every row at its defaults, on e's device; e owns
 * it: tbf_engine_destroy releases the ones still alive.  -22: a NULL pointer, n_curves out of range,
 * n_rows == 0.  A host-only engine validates, then returns -19.  -12 when the device cannot hold
 * the tables. */
int tbf_comp_create (tbf_engine* e, uint32_t n_rows, const tbf_comp_config* cfg, tbf_comp** out);
int tbf_comp_destroy (tbf_comp* comp);
/* The g of the rows `rows` (host memory, n of them; NULL: all rows, n ignored) is 1.0f again,
 * ordered on `stream` (NULL: the engine's own); their parameters stay.  -22: a row index >= n_rows. */
int tbf_comp_reset (tbf_comp* comp, uint32_t n, const uint32_t* rows, void* stream);
/* New points pts[0 .. 768] for curve `curve`.  Ordered on `stream` (NULL: the engine's own) as
 * tbf_comp_reset is: it takes effect from the next tbf_comp_device on, and every g is kept.  The
 * upload is staged in the compressor's own tables, and the call waits for `stream` before it returns,
 * so the staging outlives the copy and the caller's array is free at once.  Every point is checked
 * before anything changes: -22 (see above) leaves the curve as it was. */
int tbf_comp_curve_set (tbf_comp* comp, uint32_t curve, const float* pts, void* stream);
/* New parameters for the rows `rows` (n of them; NULL: all rows in order, n ignored): row k of the
 * list takes params[k].  Ordered, staged and waited for as tbf_comp_curve_set; every g is kept.
 * Every row is checked before anything changes: -22 leaves every row as it was. */
int tbf_comp_rows_set (tbf_comp* comp, uint32_t n, const uint32_t* rows, const tbf_comp_row* params, void* stream);
/* The read-back, from the host's tables: no wait. */
int tbf_comp_curve_get (const tbf_comp* comp, uint32_t curve, float* pts);
int tbf_comp_row_get (const tbf_comp* comp, uint32_t row, tbf_comp_row* out);
/* One call: the compressor's n_rows rows of d_L / d_R (device memory, row r at r * in_stride floats;
 * any 4-byte-aligned pointers and odd strides; d_L == d_R allowed) into d_outL / d_outR (row r at
 * r * out_stride floats) on `stream` (NULL: the engine's own), ordered as tbf_render_device.  The key
 * pair d_keyL / d_keyR (row r at r * key_stride floats; d_keyL == d_keyR allowed) is optional: both
 * NULL, and the input is its own key, or both set.  Row r takes counts[r] <= frames frames (counts:
 * host memory, uploaded before the call returns, for which the call waits for `stream`; NULL:
 * `frames` each, and no wait); a row with count 0 keeps its g.  Output rows are written in [0, count)
 * and left alone behind it; the inputs and the key are only read.  d_meters (device memory, or NULL:
 * nothing is written) takes one tbf_comp_meter for every row.  Calls on one compressor are the
 * caller's to order.  -22, with a tbf_last_error that names the argument: a NULL pointer, one key
 * pointer without the other, a stride < frames, a misaligned pointer, counts[r] > frames, an output
 * that overlaps an input, a key or the other output.  Validation comes first: a refused call moves no
 * state. */
int tbf_comp_device (tbf_comp* comp, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames, const float* d_keyL,
                     const float* d_keyR, uint64_t key_stride, float* d_outL, float* d_outR, uint64_t out_stride, const uint32_t* counts,
                     tbf_comp_meter* d_meters, void* stream);
/* The designer (see above) into pts[0 .. 768].  Needs no engine.  -22: a NULL pts, or a threshold,
 * ratio or knee outside its range, NaN included; the error names the argument. */
int tbf_comp_curve_design (double threshold_db, double ratio, double knee_db, float* pts);
/* test hook: the host restatement of the definition on one row, from the header the kernel is built
 * from (csrc/tbf_comp.h): n frames of L / R (L == R allowed) keyed by keyL / keyR (both NULL: by
 * themselves) through the curve pts[769] with the coefficients and the make-up, behind *g (read and
 * then replaced), into outL / outR, and every g[n] into gains when that is not NULL.  The curve and
 * the parameters are checked as the setters check them (the error names row 0).  Needs no engine
 * and no device. */
int tbf_debug_comp_ref (const float* pts, float attack, float release, float makeup, const float* L, const float* R, const float* keyL,
                        const float* keyR, uint64_t n, float* g, float* outL, float* outR, float* gains);
/* test hook: t for n levels (each >= 0 and not NaN, else -22) on the curve pts[769].  No engine. */
int tbf_debug_comp_lookup (const float* pts, const float* levels, uint64_t n, float* t);
/* test hook: how k_comp lays a compressor of n_rows rows and n_curves curves out: the rows of a
 * wave, the frames of a row staged in LDS at a time, and the workgroup's LDS bytes.  No layout
 * changes a bit.  Any out pointer may be NULL.  -22: n_rows == 0 or n_curves out of range. */
int tbf_debug_comp_grid (uint32_t n_rows, uint32_t n_curves, uint32_t* rows_per_wave, uint32_t* tile_frames, uint32_t* lds_bytes);
/* k_comp's own time, as tbf_debug_loudness_time: one launch per call that took frames */
int tbf_debug_comp_time (tbf_comp* comp, int32_t enable, double* ms, uint64_t* launches);

int tbf_synchronize (tbf_engine* e);
/* Which exact-but-slow paths the kernels took since the engine's first render (cumulative,
 * informational; the results are bit-identical either way).  Waits for the engine's
 * own stream and the pipelined stage streams; a caller rendering on its own stream must
 * synchronize that stream first. */
#define TBF_PATH_VIB_SERIAL 1u   /* vibrato scatter: lane-serial replay (src/vibrato.cpp:380-409) */
#define TBF_PATH_WH_ANGLE 2u     /* whirl rotor angles: literal fmod recurrence (src/whirl.cpp:1428-1429) */
#define TBF_PATH_WH_MOTION 4u    /* whirl ring adds: sample-serial replay (src/whirl.cpp:1432-1469) */
#define TBF_PATH_RV_PHASE 8u     /* reverb LFO phases: literal recurrence + sin (src/reverb.cpp:479-496) */
#define TBF_PATH_RV_WINDOW 16u   /* reverb tap outside the staged window: direct ring reads */
#define TBF_PATH_RV_SYNC 32u     /* not a path but a failure: a wave of k_rv_core_lds gave up waiting for a
                                  * neighbour's phase (the kernel ends instead of hanging); the output is wrong */
int tbf_error_flags (tbf_engine* e, uint32_t* flags);
/* read back the wave bank of a template (wheels 1..256 concatenated) for checks */
int tbf_template_bank (tbf_engine* e, uint32_t tpl_id, float* out, uint64_t cap, uint32_t* lens256);

/* ---- test hooks (host only; used by the parity tests to pin the control plane) ---- */
/* play-matrix entries of one key (keyContrib, src/tonegen.cpp:1122-1213) */
int tbf_debug_contrib (tbf_engine* e, uint32_t tpl_id, int32_t key, int16_t* wheel, int16_t* bus, float* level,
                       uint32_t cap);
/* the program the instance's next block plays unless its control changes (the persistent
 * pool entry, read back from the device after synchronizing): 9 floats per instruction
 * as tbf_debug_render_program; works with either control path */
int tbf_debug_device_program (tbf_engine* e, uint32_t inst, float* entries9, uint32_t cap);
/* host control time: wall-clock the render calls spent stepping the control plane
 * (events, message queues, active lists, routing, per-block programmes) since the last
 * reset, and the blocks it covered */
int tbf_debug_host_time (tbf_engine* e, int32_t reset, double* ms, uint64_t* blocks);
/* self-check of the host worker pool the control plane's parallel sections run on: jobs
 * of 1..40 tasks back to back (jobs of them), each task counted; returns the number of
 * jobs in which a task ran other than exactly once (0: all good) */
int tbf_debug_pool_check (uint32_t jobs);
/* the cfg-derived HBM layout: the compact whirl ring window (512 / 1024 / 2048 samples
 * per ring, from the geometry's largest write-ahead) and the reverb slab length */
int tbf_debug_layout (const tbf_engine* e, uint32_t* wring_len, float* max_ahead, uint32_t* slab_len);
/* the geometry's smallest whirl write-ahead in samples (the nearest a motion's ring add
 * lands to its own sample) and the bound under which a chain that runs the whirl is
 * refused (one 64-sample sub-block plus rounding slack) */
int tbf_debug_whirl_lead (const tbf_engine* e, float* min_ahead, float* bound);
/* blocks per render chunk: with control deltas (64) and without (TBF_STEADY_CHUNK, up to 2048) */
int tbf_debug_chunks (const tbf_engine* e, uint32_t* delta_blocks, uint32_t* steady_blocks);
/* chunks with events since the engine was created, by the front end that stepped them:
 * the device's (k_front) and the host's */
int tbf_debug_front_chunks (const tbf_engine* e, uint64_t* device_chunks, uint64_t* host_chunks);
/* test hook: launches of each kernel variant since the engine was created, counted on the
 * host where the engine launches a stage, from the fields the launch switches on.  Writes
 * min (cap, TBF_LAUNCH_KINDS) counts in the order below and returns TBF_LAUNCH_KINDS; a
 * host engine (device -1) launches nothing and reports zeros; an effects-only engine
 * (TBF_CHAIN_FX*) reports zero for both k_tonegen kinds. */
enum {
	TBF_LAUNCH_TONEGEN        = 0, /* k_tonegen, one block range per instance */
	TBF_LAUNCH_TONEGEN_RANGES = 1, /* k_tonegen, an instance's blocks split over several waves */
	TBF_LAUNCH_RV_CORE        = 2, /* k_rv_core, the streaming reverb network */
	TBF_LAUNCH_RV_CORE_LDS    = 3, /* k_rv_core_lds */
	TBF_LAUNCH_WHIRL          = 4, /* k_whirl, in any output mode (whirl_out, rotor rows) */
	TBF_LAUNCH_WHIRL_SPLIT    = 5, /* k_whirl_split, likewise */
	TBF_LAUNCH_KINDS          = 6
};
int tbf_debug_launches (const tbf_engine* e, uint64_t* counts, uint32_t cap);
/* test hook: k_rv_pre launches since the engine was created that ran ahead, on the k_whirl
 * stream beside the previous chunk's k_rv_post (TBF_PRE_AHEAD=1; 0 otherwise) */
int tbf_debug_pre_ahead (const tbf_engine* e, uint64_t* launches);
/* test hook: device memory the engine holds now.  instance_bytes: the bytes allocated for
 * the arrays whose size is a function of the instance count alone (st, wring, rslab, tgc,
 * cst, the persistent slots of the program pool, the control pool ctl and its index table
 * ctlIdx, the cabinet convolver's history when a cabinet is set and the rate converter's when one is set).  The delta part of the program pool is left out: under device control it grows
 * with the deltas of a call, and it grows by a quarter more than asked for.  stage_bytes:
 * the stage buffers mid0 / mid1 / mid2 / rvA / rvB.  Either pointer may be NULL; a host-only
 * engine reports zeros. */
int tbf_debug_device_bytes (const tbf_engine* e, uint64_t* instance_bytes, uint64_t* stage_bytes);
/* the longest render chunk without control deltas, in blocks (64 .. 2048, default 512).
 * The stage buffers hold one chunk per instance (56 B per instance and sample at the
 * default stage groups: 15 GB at 4096 instances and 512 blocks, 60 GB at 2048) and
 * grow to the longest chunk a call makes, so this bounds the engine's HBM footprint; longer
 * chunks spread each launch's state traffic over more samples.  The
 * value is clamped to what the device can hold for the instances added so far (halved
 * until the buffers fit the free memory plus the buffers held now), and a render that
 * still cannot allocate them halves it again (tbf_debug_chunks reports the value in
 * effect).  Takes effect at the next render (buffers larger than the new value are freed
 * then); returns the value in effect, or < 0 on error.  Renders are bit-identical at every
 * value. */
int tbf_set_steady_chunk (tbf_engine* e, uint32_t blocks);
/* test hook: set the reverb vibrato phase of line 0..7 of channel ch (b_reverb vib[ch][line],
 * src/reverb.cpp:479-496) of an instance, effective from the next block; parity tests use
 * it to place a phase just below a power of two (a binade crossing inside a launch) */
int tbf_debug_reverb_phase (tbf_engine* e, uint32_t inst, int32_t ch, int32_t line, double value);
/* envelopes (9 x 128 each) and key-compression table (128) of a template */
int tbf_debug_tables (tbf_engine* e, uint32_t tpl_id, float* attack, float* release, float* keycomp);
/* run one block of the tonegen control plane for an instance and return the core
 * program: per entry {wheel, env, row, sg, pg, vg, nsg, npg, nvg} as 9 floats */
int tbf_debug_step (tbf_engine* e, uint32_t inst, float* entries9, uint32_t cap);
/* the core program the instance's next rendered block uses, after the control-plane
 * step a render makes for that block (which steps only when something changed) */
int tbf_debug_render_program (tbf_engine* e, uint32_t inst, float* entries9, uint32_t cap);
/* an instance's host control state: odClean, odA, odC, rvG, revOpt, revSelect, whBypass,
 * newRouting, swellPedalGain, percEnabled, percIsSoft, percIsFast, percSendBus, vibTable,
 * vibMixed, percDrawbarGain, drawBarGain[27], the whirl's haT haF haQ haG hbT hbF hbQ hbG
 * hornAcc hornDec drumAcc drumDec hnBrakePos drBrakePos; returns the count (57) */
int tbf_debug_control (tbf_engine* e, uint32_t inst, double* out, uint32_t cap);
/* the kernel's exact shortcuts of serial recurrences, evaluated on the host (same source,
 * csrc/tbf_exact.h): op 0 phase_run (in: v0, d, m -> out: ok, D), op 1 cnt_adv (in: c0,
 * d, n -> out: count), op 2 wrap1 (in: x, -, - -> out: fmod (x, 1)), op 3 xorshift
 * dither jump (in: x0, k, - -> out: jump-table state, k literal steps), op 4 cached
 * phase steps along 4096 sub-blocks (in: v0, d, m -> out: mismatches vs phase_run, cache
 * hits), op 5 glibc rand() jump (in: seed, k, - -> out: next draw after GlibcRand::discard
 * (k), after k literal draws); n records */
int tbf_debug_exact (int32_t op, const double* in3, double* out2, uint32_t n);
/* per-stage kernel timing with HIP events on each launch's stream: enable 1 / -1 turns
 * recording on / off (1: as rendered, launches of neighbouring chunks overlapping; 2:
 * with the cross-chunk pipelining off, each kernel alone on the GPU); 0 returns the
 * summed milliseconds and launch counts of the six stage kernels k_tonegen, k_mixpre,
 * k_rv_pre, k_rv_core, k_rv_post, k_whirl since the last query (ms6[6], count6[6]) */
int tbf_debug_kernel_times (tbf_engine* e, int32_t enable, double* ms6, uint32_t* count6);
/* PMC calibration: op 0 streams n doubles from d_buf (8 B/lane reads, the reverb ring
 * pattern), op 1 writes them; ops 2 / 3 the same starting 64 B into a cache line (n >= 16);
 * op 4 (test hook for csrc/tbf_sin.h): d_buf holds n inputs x followed by room for 6 n
 * results: tbf_sin (x), sin (x), tbf_sin2's two results for (x, the input n / 2 further on),
 * the asin fast path and asin (x clamped to [-1, 1]); enqueued on `stream` (NULL = legacy
 * default stream) */
int tbf_debug_calibrate (int32_t op, void* d_buf, uint64_t n_doubles, void* stream);

#ifdef __cplusplus
}
#endif
#endif
