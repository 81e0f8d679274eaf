/*
 * tbf_mix.cpp -- the host side of the mixdown stage: tbf_mix_device, the tbf_render_mix* /
 * tbf_process_mix* calls and the tbf_debug_mix* hooks.
 *
 * A post-stage on two float32 planes (include/tbf.h): k_mix
 * (csrc/tbf_mix.hip) sums groups of rows into stereo buses, each bus one serial fmaf chain over
 * its member rows in ascending row order.  The stage has no instance state.  The caller's rows
 * are checked and turned into a bus-sorted member list here (buildList), which tbf_debug_mix_ref
 * walks on the host and the device calls upload.  tbf_mix_device runs the stage alone on the
 * caller's planes.  The render and process calls render the engine-rate pair through the
 * ordinary render path (plainRender, csrc/tbf_engine.cpp) into engine scratch
 * (tbf_engine.rotBuf), 8 B per instance and sample, cut into pieces of at most TBF_STAGE_PIECE
 * blocks, and k_mix follows each piece on the call's stream, writing at the piece's frame offset.
 * A bus sample depends on its own frame alone, so the pieces deliver what one call delivers.
 * The host-buffer calls mix into device staging and copy the bus rows out once per piece.
 * Everything is allocated before the first piece renders: -12 renders nothing.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_engine_impl.h"
#include "tbf_mix.h"

extern "C" int tbf_launch_mix (const tbf_mix_launch* P, hipStream_t stream);

using namespace tbf;

namespace {

/* the bus-sorted member list of a call's rows */
struct List {
	std::vector<uint32_t>       off; /* n_buses + 1 */
	std::vector<tbf_mix_member> mem;
};

/* The rows' own checks, then the list: a counting sort by bus, which keeps the rows ascending
 * within each bus.  counts NULL: every row holds `frames`. */
int buildList (uint32_t nRows, const tbf_mix_row* rows, const uint32_t* counts, uint32_t frames, uint32_t nBuses, List& out)
{
	out.off.assign ((size_t)nBuses + 1, 0u);
	for (uint32_t r = 0; r < nRows; r++) {
		if (counts && counts[r] > frames)
			return fail (-22, "mix: counts[" + std::to_string (r) + "] above frames");
		const tbf_mix_row& w = rows[r];
		if (w.bus == TBF_MIX_NONE)
			continue;
		if (nBuses == 0)
			return fail (-22, "mix: n_buses is 0 while rows[" + std::to_string (r) + "] names a bus");
		if (w.bus >= nBuses)
			return fail (-22, "mix: rows[" + std::to_string (r) + "].bus " + std::to_string (w.bus) + " is no bus of n_buses " +
			                      std::to_string (nBuses));
		if (!std::isfinite (w.ll) || !std::isfinite (w.lr) || !std::isfinite (w.rl) || !std::isfinite (w.rr))
			return fail (-22, "mix: rows[" + std::to_string (r) + "] has a non-finite coefficient");
		out.off[w.bus + 1]++;
	}
	for (uint32_t b = 0; b < nBuses; b++)
		out.off[b + 1] += out.off[b];
	out.mem.resize (out.off[nBuses]);
	std::vector<uint32_t> at (out.off.begin (), out.off.end () - 1);
	for (uint32_t r = 0; r < nRows; r++) {
		const tbf_mix_row& w = rows[r];
		if (w.bus != TBF_MIX_NONE)
			out.mem[at[w.bus]++] = {r, counts ? counts[r] : frames, w.ll, w.lr, w.rl, w.rr};
	}
	return 0;
}

/* a tbf_mix_out for rows of `frames` frames */
int outArgs (const tbf_mix_out* o, uint64_t frames, bool device)
{
	if (!o || !o->L || !o->R)
		return fail (-22, "null argument");
	if (o->stride < frames)
		return fail (-22, "mix: out stride smaller than frames");
	if (device && (((uintptr_t)o->L | (uintptr_t)o->R) & 3u))
		return fail (-22, "mix: device pointer not 4-byte aligned");
	return 0;
}

/* the two output planes against each other and against input rows (in: nin planes of inRows rows) */
int rangesApart (const tbf_mix_out* o, uint64_t nBuses, uint64_t frames, const float* const* in, int nin, uint64_t inRows,
                 uint64_t inStride, uint64_t inFrames)
{
	Span sp[4]; /* the inputs (nin <= 2), which may alias each other, then the two bus planes */
	for (int k = 0; k < nin; k++)
		sp[k] = rowsSpan (in[k], inRows, inStride * 4, inFrames * 4);
	sp[nin]     = rowsSpan (o->L, nBuses, o->stride * 4, frames * 4);
	sp[nin + 1] = rowsSpan (o->R, nBuses, o->stride * 4, frames * 4);
	return anyOverlap (sp, nin + 2, nin) ? fail (-22, "mix: input rows and output planes overlap") : 0;
}

/* The checks of the render and process calls and the list, all before anything renders or steps
 * (in: the effects-only calls' input rows); pointers are compared on the host only. */
int renderArgs (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, bool fx, const float* in, uint64_t inStride,
                const tbf_mix_row* rows, uint32_t nBuses, const tbf_mix_out* o, bool device, List& list)
{
	if (!e || (fx && !in) || (nev && !ev))
		return fail (-22, "null argument");
	const uint32_t n = (uint32_t)e->inst.size ();
	if (n && !rows)
		return fail (-22, "null argument");
	const uint64_t per = (uint64_t)nblocks * TBF_BLK;
	if (int rc = outArgs (o, per, device))
		return rc;
	if (fx != chainFx (e->cfg.chain_mode))
		return fail (-22, fx ? "tbf_process_mix* needs an effects-only engine (TBF_CHAIN_FX*)"
		                     : "effects-only engine (TBF_CHAIN_FX*) has no tone generator to render: use tbf_process_mix*");
	if (per > UINT32_MAX)
		return fail (-22, "call too long: the counts are 32-bit");
	if (fx && inStride < per)
		return fail (-22, "in_stride smaller than nblocks*128");
	if (device && fx && ((uintptr_t)in & 3u))
		return fail (-22, "mix: device pointer not 4-byte aligned");
	if (int rc = buildList (n, rows, nullptr, (uint32_t)per, nBuses, list))
		return rc;
	if (int rc = rangesApart (o, nBuses, per, &in, fx ? 1 : 0, n, inStride, per))
		return rc;
	if (int rc = eventsInOrder (ev, nev))
		return rc;
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) cannot render");
	return 0;
}

/* The list on the device.  It is read from host vectors of this call, so the stream is waited
 * for before they go. */
int uploadList (tbf_engine* e, const List& list, hipStream_t s, tbf_mix_launch& P)
{
	tbf_engine::Mix& c = e->mix;
	if (c.busOff.ensure (list.off.size ()) || c.members.ensure (list.mem.size ())) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (mix list)");
	}
	HIPCHK (hipMemcpyAsync (c.busOff.p, list.off.data (), list.off.size () * sizeof (uint32_t), hipMemcpyHostToDevice, s));
	if (!list.mem.empty ())
		HIPCHK (hipMemcpyAsync (c.members.p, list.mem.data (), list.mem.size () * sizeof (tbf_mix_member), hipMemcpyHostToDevice, s));
	HIPCHK (hipStreamSynchronize (s));
	P.busOff  = c.busOff.p;
	P.members = c.members.p;
	return 0;
}

/* k_mix over nBuses buses on s, in launches of at most TBF_MIX_MAX_BUSES; P.busBase / P.nBuses / P.group are set here */
int launchStage (tbf_engine* e, tbf_mix_launch P, uint32_t nBuses, hipStream_t s)
{
	tbf_engine::Mix& c = e->mix;
	if (nBuses == 0 || P.frames == 0)
		return 0;
	StageTimer::Guard tg (c.timer, s, "mix"); /* tbf_debug_mix_time: k_mix between two events on its stream */
	if (int rc = tg.begin ())
		return rc;
	P.group = mix_frames_per_lane (P.frames, nBuses);
	for (uint32_t b0 = 0; b0 < nBuses; b0 += TBF_MIX_MAX_BUSES) {
		P.busBase = b0;
		P.nBuses  = std::min (TBF_MIX_MAX_BUSES, nBuses - b0);
		if (tbf_launch_mix (&P, s))
			return fail (-5, std::string ("k_mix launch failed: ") + hipGetErrorString (hipGetLastError ()));
	}
	if (int rc = tg.end ())
		return rc;
	c.launches++;
	return 0;
}

/* One render or process call, after renderArgs.  host: o's planes are host memory, filled through
 * the engine's staging on its own stream s, and the call returns with them complete. */
int renderMix (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* in, uint64_t inStride,
               const List& list, uint32_t nBuses, const tbf_mix_out& o, hipStream_t s, bool host)
{
	HIPCHK (hipSetDevice (e->cfg.device));
	tbf_engine::Mix& c = e->mix;
	const uint32_t   n = (uint32_t)e->inst.size ();
	if (int rc = engineDevice (e))
		return rc;
	if (nblocks == 0 || (n == 0 && nBuses == 0)) /* nothing renders and no event applies, as in every render call */
		return 0;
	const uint32_t piece = std::min (nblocks, TBF_STAGE_PIECE);
	const size_t   per = (size_t)nblocks * TBF_BLK, pframes = (size_t)piece * TBF_BLK, plane = (size_t)n * pframes;
	const size_t   oplane = (size_t)nBuses * pframes;
	if (e->rotBuf.ensure (2 * plane) || (host && (c.hostOut.ensure (2 * oplane) || (in && e->extBuf.ensure ((size_t)n * per))))) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (mix scratch: 8 B per instance and sample of a piece)");
	}
	tbf_mix_launch P;
	memset (&P, 0, sizeof (P));
	if (int rc = uploadList (e, list, s, P))
		return rc;
	const float* dIn = in;
	if (host && in && n) {
		if (int rc = stageHostInput (e->extBuf.p, in, inStride, per, n, s))
			return rc;
		dIn      = e->extBuf.p;
		inStride = per;
	}
	float* const pl = e->rotBuf.p, * const pr = e->rotBuf.p + plane;
	P.in[0]    = pl;
	P.in[1]    = pr;
	P.inStride = pframes;
	for (Pieces pc (ev, nev, nblocks, piece); pc.next ();) {
		const uint32_t p0 = pc.p0, len = pc.len;
		if (n)
			if (int rc = plainRender (e, len, pc.npe ? pc.pe : nullptr, pc.npe, dIn ? dIn + (size_t)p0 * TBF_BLK : nullptr, inStride,
			                          pl, pr, pframes, s))
				return rc;
		const size_t off = (size_t)p0 * TBF_BLK, rowFrames = (size_t)len * TBF_BLK;
		P.out[0]    = host ? c.hostOut.p : o.L + off;
		P.out[1]    = host ? c.hostOut.p + oplane : o.R + off;
		P.outStride = host ? rowFrames : o.stride;
		P.frames    = (uint32_t)rowFrames; /* the members' counts are the call's: k_mix takes min (count, frames) */
		if (int rc = launchStage (e, P, nBuses, s))
			return rc;
		if (host && nBuses) { /* the staging is the next piece's too: wait for the copies */
			HIPCHK (hipMemcpy2DAsync (o.L + off, o.stride * 4, P.out[0], rowFrames * 4, rowFrames * 4, nBuses, hipMemcpyDeviceToHost, s));
			HIPCHK (hipMemcpy2DAsync (o.R + off, o.stride * 4, P.out[1], rowFrames * 4, rowFrames * 4, nBuses, hipMemcpyDeviceToHost, s));
			HIPCHK (hipStreamSynchronize (s));
		}
	}
	return 0;
}

} // namespace

extern "C" {

int tbf_mix_device (tbf_engine* e, uint32_t n_rows, const float* d_L, const float* d_R, uint64_t in_stride, uint32_t frames,
                    const uint32_t* counts, const tbf_mix_row* rows, uint32_t n_buses, const tbf_mix_out* out, void* stream)
{
	if (!e || !d_L || !d_R || (n_rows && !rows))
		return fail (-22, "null argument");
	if (int rc = outArgs (out, frames, true))
		return rc;
	if (((uintptr_t)d_L | (uintptr_t)d_R) & 3u)
		return fail (-22, "mix: device pointer not 4-byte aligned");
	if (in_stride < frames)
		return fail (-22, "in_stride smaller than frames");
	List list;
	if (int rc = buildList (n_rows, rows, counts, frames, n_buses, list))
		return rc;
	const float* const in[2] = {d_L, d_R};
	if (int rc = rangesApart (out, n_buses, frames, in, 2, n_rows, in_stride, frames))
		return rc;
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) has no device to mix on");
	HIPCHK (hipSetDevice (e->cfg.device));
	hipStream_t const s = streamOr (stream, e->stream);
	if (n_buses == 0 || frames == 0)
		return 0;
	tbf_mix_launch P;
	memset (&P, 0, sizeof (P));
	if (int rc = uploadList (e, list, s, P))
		return rc;
	P.in[0]     = d_L;
	P.in[1]     = d_R;
	P.inStride  = in_stride;
	P.out[0]    = out->L;
	P.out[1]    = out->R;
	P.outStride = out->stride;
	P.frames    = frames;
	return launchStage (e, P, n_buses, s);
}

int tbf_render_mix (tbf_engine* e, uint32_t nblocks, const tbf_mix_row* rows, uint32_t n_buses, const tbf_mix_out* out)
{
	List list;
	if (int rc = renderArgs (e, nblocks, nullptr, 0, false, nullptr, 0, rows, n_buses, out, false, list))
		return rc;
	return renderMix (e, nblocks, nullptr, 0, nullptr, 0, list, n_buses, *out, e->stream, true);
}

int tbf_render_mix_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const tbf_mix_row* rows,
                           uint32_t n_buses, const tbf_mix_out* out, void* stream)
{
	List list;
	if (int rc = renderArgs (e, nblocks, ev, nev, false, nullptr, 0, rows, n_buses, out, true, list))
		return rc;
	return renderMix (e, nblocks, ev, nev, nullptr, 0, list, n_buses, *out, streamOr (stream, e->stream), false);
}

int tbf_process_mix (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t inStride, const tbf_mix_row* rows, uint32_t n_buses,
                     const tbf_mix_out* out)
{
	List list;
	if (int rc = renderArgs (e, nblocks, nullptr, 0, true, in, inStride, rows, n_buses, out, false, list))
		return rc;
	return renderMix (e, nblocks, nullptr, 0, in, inStride, list, n_buses, *out, e->stream, true);
}

int tbf_process_mix_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn, uint64_t inStride,
                            const tbf_mix_row* rows, uint32_t n_buses, const tbf_mix_out* out, void* stream)
{
	List list;
	if (int rc = renderArgs (e, nblocks, ev, nev, true, dIn, inStride, rows, n_buses, out, true, list))
		return rc;
	return renderMix (e, nblocks, ev, nev, dIn, inStride, list, n_buses, *out, streamOr (stream, e->stream), false);
}

int tbf_debug_mix_ref (uint32_t n_rows, const float* L, const float* R, uint64_t in_stride, uint32_t frames, const uint32_t* counts,
                       const tbf_mix_row* rows, uint32_t n_buses, const tbf_mix_out* out)
{
	if ((n_rows && (!L || !R || !rows)))
		return fail (-22, "null argument");
	if (int rc = outArgs (out, frames, false))
		return rc;
	if (in_stride < frames)
		return fail (-22, "in_stride smaller than frames");
	List list;
	if (int rc = buildList (n_rows, rows, counts, frames, n_buses, list))
		return rc;
	const float* const in[2] = {L, R};
	if (int rc = rangesApart (out, n_buses, frames, in, 2, n_rows, in_stride, frames))
		return rc;
	for (uint32_t b = 0; b < n_buses; b++) {
		float* const ol = out->L + (uint64_t)b * out->stride, * const orr = out->R + (uint64_t)b * out->stride;
		for (uint32_t j = 0; j < frames; j++)
			ol[j] = orr[j] = 0.0f;
		for (uint32_t m = list.off[b]; m < list.off[b + 1]; m++) {
			const tbf_mix_member& w = list.mem[m];
			const float* const    l = L + (uint64_t)w.row * in_stride, * const r = R + (uint64_t)w.row * in_stride;
			for (uint32_t j = 0; j < w.count; j++)
				mix_term (w.ll, w.lr, w.rl, w.rr, l[j], r[j], ol[j], orr[j]);
		}
	}
	return 0;
}

int tbf_debug_mix_grid (uint32_t frames, uint32_t n_buses, uint32_t* frames_per_lane, uint32_t* tile_frames, uint32_t* slice_buses)
{
	const uint32_t g = mix_frames_per_lane (frames, n_buses);
	if (frames_per_lane)
		*frames_per_lane = g;
	if (tile_frames)
		*tile_frames = TBF_MIX_LANES * g;
	if (slice_buses)
		*slice_buses = TBF_MIX_MAX_BUSES;
	return 0;
}

int tbf_debug_mix_time (tbf_engine* e, int32_t enable, double* ms, uint64_t* launches)
{
	if (!e)
		return fail (-22, "null argument");
	return e->mix.timer.query (enable, ms, launches);
}

} /* extern "C" */
