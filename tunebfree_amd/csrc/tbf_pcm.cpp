/*
 * tbf_pcm.cpp -- the host side of the PCM output stage: tbf_pcm_convert_device, the
 * tbf_render_pcm* / tbf_process_pcm* calls and the tbf_debug_pcm* hooks.
 *
 * A post-stage on two float32 planes (include/tbf.h): k_pcm
 * (csrc/tbf_pcm.hip) packs them into interleaved int16 / int24 / float32 frames and meters them.
 * The stage has no instance state.  tbf_pcm_convert_device runs it alone on the caller's planes.
 * The render and process calls render the engine-rate pair through the ordinary render path
 * (plainRender, csrc/tbf_engine.cpp) into engine scratch (tbf_engine.rotBuf), 8 B per instance and
 * sample, cut into pieces of at most TBF_STAGE_PIECE blocks so the scratch never exceeds
 * n x TBF_STAGE_PIECE x 128 x 8 B, and k_pcm follows each piece on the call's stream.  Dither is a
 * function of the frame index and the meters are integer maxima and sums, so the pieces deliver
 * what one call delivers.  The host-buffer calls convert into device staging and copy the packed
 * rows out once per piece.  Everything is allocated before the first piece renders: -12 renders
 * nothing.
 */
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/tbf.h"
#include "tbf_engine_impl.h"
#include "tbf_pcm.h"

extern "C" int tbf_launch_pcm (const tbf_pcm_launch* P, hipStream_t stream);

using namespace tbf;

namespace {

/* format, flags, stride and alignment of a tbf_pcm_out for rows of `frames` frames */
int outArgs (const tbf_pcm_out* o, uint64_t frames, bool device)
{
	if (!o || !o->out)
		return fail (-22, "null argument");
	if (o->format > TBF_PCM_F32)
		return fail (-22, "pcm: format " + std::to_string (o->format) + " does not exist");
	if (o->flags & ~TBF_PCM_DITHER)
		return fail (-22, "pcm: flags beyond TBF_PCM_DITHER");
	if ((o->flags & TBF_PCM_DITHER) && o->format != TBF_PCM_S16)
		return fail (-22, "pcm: dither is for TBF_PCM_S16 only");
	if (o->out_stride_bytes & 3u)
		return fail (-22, "pcm: out_stride_bytes is no multiple of 4");
	if (o->out_stride_bytes < frames * pcm_frame_bytes (o->format))
		return fail (-22, "pcm: out_stride_bytes smaller than a row's frames");
	if (device && (((uintptr_t)o->out | (uintptr_t)o->meters) & 3u))
		return fail (-22, "pcm: device pointer not 4-byte aligned");
	return 0;
}

/* the frames and the meters against each other and against input rows */
int rangesApart (const tbf_pcm_out* o, uint64_t rows, uint64_t frames, const float* const* in, int nin, uint64_t inStride)
{
	Span sp[4]; /* the inputs (nin <= 2), which may alias each other, then the frames and the meters */
	for (int k = 0; k < nin; k++)
		sp[k] = rowsSpan (in[k], rows, inStride * 4, frames * 4);
	sp[nin]     = rowsSpan (o->out, rows, o->out_stride_bytes, frames * pcm_frame_bytes (o->format));
	sp[nin + 1] = rowsSpan (o->meters, rows, sizeof (tbf_pcm_meter), sizeof (tbf_pcm_meter));
	return anyOverlap (sp, nin + 2, nin) ? fail (-22, "pcm: input, frame and meter ranges overlap") : 0;
}

/* The checks of the render and process calls, all before anything renders or steps (in: the
 * effects-only calls' input rows); pointers are compared on the host only. */
int renderArgs (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, bool fx, const float* in, uint64_t inStride,
                const tbf_pcm_out* o, bool device)
{
	if (!e || (fx && !in) || (nev && !ev))
		return fail (-22, "null argument");
	const uint64_t per = (uint64_t)nblocks * TBF_BLK;
	if (int rc = outArgs (o, per, device))
		return rc;
	if (fx != chainFx (e->cfg.chain_mode))
		return fail (-22, fx ? "tbf_process_pcm* needs an effects-only engine (TBF_CHAIN_FX*)"
		                     : "effects-only engine (TBF_CHAIN_FX*) has no tone generator to render: use tbf_process_pcm*");
	if (per > UINT32_MAX)
		return fail (-22, "call too long: the counts are 32-bit");
	if (fx && inStride < per)
		return fail (-22, "in_stride smaller than nblocks*128");
	if (device && fx && ((uintptr_t)in & 3u))
		return fail (-22, "pcm: device pointer not 4-byte aligned");
	if (int rc = rangesApart (o, e->inst.size (), per, &in, fx ? 1 : 0, inStride))
		return rc;
	if (int rc = eventsInOrder (ev, nev))
		return rc;
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) cannot render");
	return 0;
}

/* The rows' table on the device, where counts or dither frames differ between rows.  It is read
 * from a host vector of this call, so the stream is waited for before the vector goes. */
int uploadRows (tbf_engine* e, uint32_t n, const uint32_t* counts, const tbf_pcm_out& o, hipStream_t s, tbf_pcm_launch& P)
{
	const uint64_t* f0 = (o.flags & TBF_PCM_DITHER) ? o.row_frame0 : nullptr;
	P.rows      = nullptr;
	P.rowCounts = 0;
	if (!counts && !f0)
		return 0;
	if (e->pcm.rows.ensure (n)) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (pcm rows)");
	}
	std::vector<tbf_pcm_row> t (n);
	for (uint32_t r = 0; r < n; r++)
		t[r] = {f0 ? f0[r] : o.frame0, counts ? counts[r] : 0u, 0u};
	HIPCHK (hipMemcpyAsync (e->pcm.rows.p, t.data (), (size_t)n * sizeof (tbf_pcm_row), hipMemcpyHostToDevice, s));
	HIPCHK (hipStreamSynchronize (s));
	P.rows      = e->pcm.rows.p;
	P.rowCounts = counts != nullptr;
	return 0;
}

/* k_pcm over nRows rows on s, in launches of at most TBF_PCM_MAX_ROWS; P.rowBase / P.nRows are set here */
int launchStage (tbf_engine* e, tbf_pcm_launch P, uint32_t nRows, hipStream_t s)
{
	tbf_engine::Pcm& c = e->pcm;
	if (nRows == 0 || P.maxCount == 0)
		return 0;
	StageTimer::Guard tg (c.timer, s, "pcm"); /* tbf_debug_pcm_time: k_pcm between two events on its stream */
	if (int rc = tg.begin ())
		return rc;
	for (uint32_t r0 = 0; r0 < nRows; r0 += TBF_PCM_MAX_ROWS) {
		P.rowBase = r0;
		P.nRows   = std::min (TBF_PCM_MAX_ROWS, nRows - r0);
		if (tbf_launch_pcm (&P, s))
			return fail (-5, std::string ("k_pcm launch failed: ") + hipGetErrorString (hipGetLastError ()));
	}
	if (int rc = tg.end ())
		return rc;
	c.launches++;
	return 0;
}

tbf_pcm_launch launchOf (const tbf_pcm_out& o)
{
	tbf_pcm_launch P;
	memset (&P, 0, sizeof (P));
	P.frame0U = o.frame0;
	P.format  = o.format;
	P.flags   = o.flags;
	P.seed    = o.seed;
	return P;
}

/* One render or process call, after renderArgs.  host: o's out and meters are host memory, filled
 * through the engine's staging on its own stream s, and the call returns with them complete. */
int renderPcm (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* in, uint64_t inStride,
               const tbf_pcm_out& o, hipStream_t s, bool host)
{
	HIPCHK (hipSetDevice (e->cfg.device));
	tbf_engine::Pcm& c = e->pcm;
	const uint32_t   n = (uint32_t)e->inst.size ();
	if (int rc = engineDevice (e))
		return rc;
	if (n == 0 || nblocks == 0) /* nothing renders and no event applies, as in every render call */
		return 0;
	const uint32_t piece = std::min (nblocks, TBF_STAGE_PIECE), fb = pcm_frame_bytes (o.format);
	const size_t   per = (size_t)nblocks * TBF_BLK, pframes = (size_t)piece * TBF_BLK, plane = (size_t)n * pframes;
	if (e->rotBuf.ensure (2 * plane) ||
	    (host && (c.hostOut.ensure (plane * fb) || (o.meters && c.hostMeters.ensure (n)) || (in && e->extBuf.ensure ((size_t)n * per))))) {
		(void)hipGetLastError ();
		return fail (-12, "out of device memory (pcm scratch: 8 B per instance and sample of a piece)");
	}
	tbf_pcm_launch P = launchOf (o);
	if (int rc = uploadRows (e, n, nullptr, o, s, P))
		return rc;
	const float* dIn = in;
	if (host && in) {
		if (int rc = stageHostInput (e->extBuf.p, in, inStride, per, n, s))
			return rc;
		dIn      = e->extBuf.p;
		inStride = per;
	}
	float* const pl = e->rotBuf.p, * const pr = e->rotBuf.p + plane;
	P.in[0]    = pl;
	P.in[1]    = pr;
	P.inStride = pframes;
	P.meters   = o.meters ? (host ? c.hostMeters.p : o.meters) : nullptr;
	if (P.meters)
		HIPCHK (hipMemsetAsync (P.meters, 0, (size_t)n * sizeof (tbf_pcm_meter), s));
	for (Pieces pc (ev, nev, nblocks, piece); pc.next ();) {
		const uint32_t p0 = pc.p0, len = pc.len;
		if (int rc = plainRender (e, len, pc.npe ? pc.pe : nullptr, pc.npe, dIn ? dIn + (size_t)p0 * TBF_BLK : nullptr, inStride, pl,
		                          pr, pframes, s))
			return rc;
		const size_t off = (size_t)p0 * TBF_BLK * fb, rowBytes = (size_t)len * TBF_BLK * fb;
		P.out            = host ? c.hostOut.p : (unsigned char*)o.out + off;
		P.outStride      = host ? rowBytes : o.out_stride_bytes;
		P.frameOff       = (uint64_t)p0 * TBF_BLK;
		P.countU = P.maxCount = len * TBF_BLK;
		if (int rc = launchStage (e, P, n, s))
			return rc;
		if (host) { /* the staging is the next piece's too: wait for the copy */
			HIPCHK (hipMemcpy2DAsync ((unsigned char*)o.out + off, o.out_stride_bytes, c.hostOut.p, rowBytes, rowBytes, n,
			                          hipMemcpyDeviceToHost, s));
			HIPCHK (hipStreamSynchronize (s));
		}
	}
	if (host && o.meters) {
		HIPCHK (hipMemcpyAsync (o.meters, c.hostMeters.p, (size_t)n * sizeof (tbf_pcm_meter), hipMemcpyDeviceToHost, s));
		HIPCHK (hipStreamSynchronize (s));
	}
	return 0;
}

template <int FMT, bool DITHER>
void refRow (uint32_t seed, uint32_t row, uint64_t frame0, const float* L, const float* R, uint64_t n, unsigned char* out, pcm_acc& m)
{
	const uint32_t fb = pcm_frame_bytes (FMT);
	for (uint64_t j = 0; j < n; j += TBF_PCM_GROUP) {
		const uint32_t nf = (uint32_t)std::min<uint64_t> (TBF_PCM_GROUP, n - j);
		uint32_t       l[4] = {0u, 0u, 0u, 0u}, r[4] = {0u, 0u, 0u, 0u}, w[8];
		memcpy (l, L + j, nf * 4u);
		memcpy (r, R + j, nf * 4u);
		const uint32_t bytes = pcm_group<FMT, DITHER> (l, r, nf, seed, row, frame0 + j, w, m);
		for (uint32_t b = 0; b < bytes; b++) /* the dwords are little-endian, whatever the host is */
			out[j * fb + b] = (unsigned char)(w[b >> 2] >> (8u * (b & 3u)));
	}
}

} // namespace

extern "C" {

int tbf_pcm_convert_device (tbf_engine* e, uint32_t n_rows, const float* d_L, const float* d_R, uint64_t in_stride,
                            uint32_t frames, const uint32_t* counts, const tbf_pcm_out* out, void* stream)
{
	if (!e || !d_L || !d_R)
		return fail (-22, "null argument");
	if (int rc = outArgs (out, frames, true))
		return rc;
	if (((uintptr_t)d_L | (uintptr_t)d_R) & 3u)
		return fail (-22, "pcm: device pointer not 4-byte aligned");
	if (in_stride < frames)
		return fail (-22, "in_stride smaller than frames");
	uint32_t most;
	if (int rc = countsMost ("pcm", counts, n_rows, frames, &most))
		return rc;
	const float* const in[2] = {d_L, d_R};
	if (int rc = rangesApart (out, n_rows, frames, in, 2, in_stride))
		return rc;
	if (e->cfg.device < 0)
		return fail (-19, "host-only engine (device -1) has no device to convert on");
	HIPCHK (hipSetDevice (e->cfg.device));
	hipStream_t const s = streamOr (stream, e->stream);
	if (n_rows == 0)
		return 0;
	tbf_pcm_launch P = launchOf (*out);
	if (int rc = uploadRows (e, n_rows, counts, *out, s, P))
		return rc;
	if (out->meters)
		HIPCHK (hipMemsetAsync (out->meters, 0, (size_t)n_rows * sizeof (tbf_pcm_meter), s));
	P.in[0]     = d_L;
	P.in[1]     = d_R;
	P.inStride  = in_stride;
	P.out       = (unsigned char*)out->out;
	P.outStride = out->out_stride_bytes;
	P.meters    = out->meters;
	P.countU    = frames;
	P.maxCount  = most;
	return launchStage (e, P, n_rows, s);
}

int tbf_render_pcm (tbf_engine* e, uint32_t nblocks, const tbf_pcm_out* out)
{
	if (int rc = renderArgs (e, nblocks, nullptr, 0, false, nullptr, 0, out, false))
		return rc;
	return renderPcm (e, nblocks, nullptr, 0, nullptr, 0, *out, e->stream, true);
}

int tbf_render_pcm_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const tbf_pcm_out* out,
                           void* stream)
{
	if (int rc = renderArgs (e, nblocks, ev, nev, false, nullptr, 0, out, true))
		return rc;
	return renderPcm (e, nblocks, ev, nev, nullptr, 0, *out, streamOr (stream, e->stream), false);
}

int tbf_process_pcm (tbf_engine* e, uint32_t nblocks, const float* in, uint64_t inStride, const tbf_pcm_out* out)
{
	if (int rc = renderArgs (e, nblocks, nullptr, 0, true, in, inStride, out, false))
		return rc;
	return renderPcm (e, nblocks, nullptr, 0, in, inStride, *out, e->stream, true);
}

int tbf_process_pcm_device (tbf_engine* e, uint32_t nblocks, const tbf_event* ev, uint32_t nev, const float* dIn,
                            uint64_t inStride, const tbf_pcm_out* out, void* stream)
{
	if (int rc = renderArgs (e, nblocks, ev, nev, true, dIn, inStride, out, true))
		return rc;
	return renderPcm (e, nblocks, ev, nev, dIn, inStride, *out, streamOr (stream, e->stream), false);
}

int tbf_debug_pcm_ref (uint32_t format, uint32_t flags, uint32_t seed, uint32_t row, uint64_t frame0, const float* L,
                       const float* R, uint64_t n, void* out, tbf_pcm_meter* meter)
{
	if (n && (!L || !R || !out))
		return fail (-22, "null argument");
	if (format > TBF_PCM_F32)
		return fail (-22, "pcm: format " + std::to_string (format) + " does not exist");
	if (flags & ~TBF_PCM_DITHER)
		return fail (-22, "pcm: flags beyond TBF_PCM_DITHER");
	if ((flags & TBF_PCM_DITHER) && format != TBF_PCM_S16)
		return fail (-22, "pcm: dither is for TBF_PCM_S16 only");
	pcm_acc              m = {{0u, 0u}, {0u, 0u}};
	unsigned char* const o = (unsigned char*)out;
	if (format == TBF_PCM_S16 && (flags & TBF_PCM_DITHER))
		refRow<TBF_PCM_S16, true> (seed, row, frame0, L, R, n, o, m);
	else if (format == TBF_PCM_S16)
		refRow<TBF_PCM_S16, false> (seed, row, frame0, L, R, n, o, m);
	else if (format == TBF_PCM_S24_3LE)
		refRow<TBF_PCM_S24_3LE, false> (seed, row, frame0, L, R, n, o, m);
	else
		refRow<TBF_PCM_F32, false> (seed, row, frame0, L, R, n, o, m);
	if (meter)
		*meter = {pcm_float (m.peak[0]), pcm_float (m.peak[1]), m.clip[0], m.clip[1]};
	return 0;
}

int tbf_debug_pcm_time (tbf_engine* e, int32_t enable, double* ms, uint64_t* launches)
{
	if (!e)
		return fail (-22, "null argument");
	return e->pcm.timer.query (enable, ms, launches);
}

} /* extern "C" */
