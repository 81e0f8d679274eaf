/*
 * tools/stage_san.cpp -- the plane stages' shared host scaffold (tunebfree_amd/csrc/tbf_stage.h)
 * under AddressSanitizer + UBSan (make -C tunebfree_amd stage_san; a CPU program, no device), over
 * seeded random cases on heap arrays of exactly the sizes used, so that one element read beyond
 * them is reported:
 *   Pieces against a restatement (refPieces): every event in exactly one piece and in order, its
 *   block counted from the piece, the events at or beyond the call's end in the last piece, the
 *   lengths summing to the call's, the caller's own pointer for the first piece and for a piece
 *   without events;
 *   overlap and anyOverlap against bytes marked in a small arena, with NULL pointers, no rows, empty
 *   rows, strides beyond a row and ranges that touch;
 *   countsMost and checkRows: the first offender is the one named, no counts means `frames`.
 * Exit code 0 and "stage_san: ok" when everything held.
 */
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../tunebfree_amd/csrc/tbf_stage.h"

using namespace tbf;

static uint32_t lcg (uint32_t& s) { return s = s * 1664525u + 1013904223u; }
static uint32_t below (uint32_t& s, uint32_t n) { return (lcg (s) >> 8) % n; }

static uint32_t g_case = 0;

#define CHECK(x)                                                                  \
	do {                                                                          \
		if (!(x)) {                                                               \
			fprintf (stderr, "stage_san: %s failed (line %d, case %u): %s\n", #x, __LINE__, g_case, tbf_last_error ()); \
			return 1;                                                             \
		}                                                                         \
	} while (0)

/* the pieces as the stages have always cut them: for event k its piece and its block there */
struct RefEvent {
	uint32_t piece, block;
};
static uint32_t refPieces (const tbf_event* ev, uint32_t nev, uint32_t nblocks, uint32_t piece, RefEvent* out)
{
	const uint32_t np = (nblocks + piece - 1u) / piece;
	for (uint32_t k = 0; k < nev; k++) {
		const uint32_t p = ev[k].block >= nblocks ? np - 1u : ev[k].block / piece;
		out[k]           = {p, ev[k].block - p * piece};
	}
	return np;
}

static int piecesCase (uint32_t& seed)
{
	static const uint32_t sizes[6] = {1u, 255u, 256u, 257u, 512u, 513u};
	const uint32_t        nblocks = sizes[below (seed, 6u)], nev = below (seed, 41u);
	const uint32_t        piece = below (seed, 4u) ? TBF_STAGE_PIECE : 1u + below (seed, nblocks);
	std::unique_ptr<tbf_event[]> ev (new tbf_event[nev]);
	std::unique_ptr<RefEvent[]>  ref (new RefEvent[nev]);
	/* in block order, some of them at or beyond the call's end */
	std::vector<uint32_t> blocks (nev);
	for (uint32_t& b : blocks)
		b = below (seed, 8u) ? below (seed, nblocks) : nblocks + below (seed, 3u);
	std::sort (blocks.begin (), blocks.end ());
	for (uint32_t k = 0; k < nev; k++) {
		memset (&ev[k], 0, sizeof (tbf_event));
		ev[k].block = blocks[k];
		ev[k].inst  = k; /* the event's name */
		ev[k].id    = (int32_t)lcg (seed);
	}
	const uint32_t np = refPieces (ev.get (), nev, nblocks, piece, ref.get ());
	uint32_t       seen = 0, pieces = 0, total = 0;
	for (Pieces pc (nev ? ev.get () : nullptr, nev, nblocks, piece); pc.next (); pieces++) {
		CHECK (pc.p0 == pieces * piece && pc.p0 == total);
		CHECK (pc.len == std::min (piece, nblocks - pc.p0));
		total += pc.len;
		if (pieces == 0 || pc.npe == 0)
			CHECK (pc.pe == (nev ? ev.get () : nullptr) + seen);
		CHECK (seen + pc.npe <= nev);
		for (uint32_t k = 0; k < pc.npe; k++, seen++) {
			CHECK (pc.pe[k].inst == seen && pc.pe[k].id == ev[seen].id);
			CHECK (ref[seen].piece == pieces && pc.pe[k].block == ref[seen].block);
			CHECK (pc.pe[k].block + pc.p0 == ev[seen].block);
		}
	}
	CHECK (pieces == np && total == nblocks && seen == nev);
	return 0;
}

/* a span's bytes marked in the arena, first byte to last: the checks compare whole ranges, the gaps
 * between the rows included.  1 when a byte was marked before. */
static int mark (std::vector<uint8_t>& arena, const unsigned char* base, const unsigned char* p, uint64_t rows, uint64_t stride,
                 uint64_t rowBytes)
{
	int hit = 0;
	if (!p || !rows || !rowBytes)
		return 0;
	for (uint64_t i = 0; i < (rows - 1u) * stride + rowBytes; i++) {
		uint8_t& b = arena[(size_t)(p - base) + i];
		hit |= b;
		b = 1u;
	}
	return hit;
}

static int spansCase (uint32_t& seed)
{
	const uint32_t                   A = 96u;
	std::unique_ptr<unsigned char[]> mem (new unsigned char[A]);
	const int                        k = 2 + (int)below (seed, 4u), nIn = (int)below (seed, 3u);
	struct Arg {
		const unsigned char* p;
		uint64_t             rows, stride, rowBytes;
	} a[5];
	Span s[5];
	for (int i = 0; i < k; i++) {
		const uint32_t kind = below (seed, 8u);
		a[i].rows     = kind == 0u ? 0u : 1u + below (seed, 3u);
		a[i].rowBytes = kind == 1u ? 0u : 1u + below (seed, 8u);
		a[i].stride   = a[i].rowBytes + (below (seed, 2u) ? below (seed, 6u) : 0u); /* at times beyond a row */
		const uint64_t len = a[i].rows ? (a[i].rows - 1u) * a[i].stride + a[i].rowBytes : 0u;
		a[i].p        = kind == 2u ? nullptr : mem.get () + below (seed, (uint32_t)(A - len + 1u));
		if (i && kind == 3u && a[i - 1].p && a[i].p) { /* touching: this one starts where the last one ends */
			const uint64_t plen = a[i - 1].rows ? (a[i - 1].rows - 1u) * a[i - 1].stride + a[i - 1].rowBytes : 0u;
			if ((size_t)(a[i - 1].p - mem.get ()) + plen + len <= A)
				a[i].p = a[i - 1].p + plen;
		}
		s[i] = rowsSpan (a[i].p, a[i].rows, a[i].stride, a[i].rowBytes);
	}
	/* pairs, then the k of them with the first nIn free to alias each other */
	bool any = false;
	for (int i = 0; i < k; i++)
		for (int j = i + 1; j < k; j++) {
			std::vector<uint8_t> arena (A, 0u);
			(void)mark (arena, mem.get (), a[i].p, a[i].rows, a[i].stride, a[i].rowBytes);
			const bool hit = mark (arena, mem.get (), a[j].p, a[j].rows, a[j].stride, a[j].rowBytes) != 0;
			CHECK (overlap (s[i], s[j]) == hit && overlap (s[j], s[i]) == hit);
			any = any || (hit && j >= nIn);
		}
	CHECK (anyOverlap (s, k, nIn) == any);
	if (nIn == 0)
		CHECK (anyOverlap (s, k) == any);
	return 0;
}

static int argsCase (uint32_t& seed)
{
	const uint32_t              n = below (seed, 9u), frames = below (seed, 50u), nRows = 1u + below (seed, 12u);
	std::unique_ptr<uint32_t[]> counts (new uint32_t[n]), rows (new uint32_t[n]);
	uint32_t                    badCount = n, badRow = n, big = 0u;
	for (uint32_t r = 0; r < n; r++) {
		counts[r] = below (seed, 6u) ? below (seed, frames + 1u) : frames + 1u + below (seed, 3u);
		rows[r]   = below (seed, 6u) ? below (seed, nRows) : nRows + below (seed, 3u);
		if (counts[r] > frames && badCount == n)
			badCount = r;
		if (rows[r] >= nRows && badRow == n)
			badRow = r;
		big = std::max (big, counts[r]);
	}
	uint32_t most = ~0u;
	CHECK (countsMost ("tag", nullptr, n, frames, &most) == 0 && most == frames);
	if (badCount == n)
		CHECK (countsMost ("tag", counts.get (), n, frames, &most) == 0 && most == big);
	else {
		CHECK (countsMost ("tag", counts.get (), n, frames, &most) == -22);
		CHECK (std::string (tbf_last_error ()) == "tag: counts[" + std::to_string (badCount) + "] above frames");
	}
	CHECK (checkRows ("tag", n, nullptr, nRows) == 0);
	if (badRow == n)
		CHECK (checkRows ("tag", n, rows.get (), nRows) == 0);
	else {
		CHECK (checkRows ("tag", n, rows.get (), nRows) == -22);
		CHECK (std::string (tbf_last_error ()) == "tag: rows[" + std::to_string (badRow) + "] " + std::to_string (rows[badRow]) +
		                                              " is no row of n_rows " + std::to_string (nRows));
	}
	return 0;
}

int main ()
{
	uint32_t seed = 20261021u;
	for (g_case = 0; g_case < 4000u; g_case++)
		if (piecesCase (seed) || spansCase (seed) || argsCase (seed))
			return 1;
	printf ("stage_san: %u cases each of pieces, spans and argument checks\n", g_case);
	printf ("stage_san: ok\n");
	return 0;
}
