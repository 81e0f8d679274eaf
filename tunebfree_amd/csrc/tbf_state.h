/*
 * tbf_state.h -- the tables of k_state_move (csrc/tbf_state.hip), shared with its host
 * side (csrc/tbf_fork.cpp).
 */
#ifndef TBF_STATE_H
#define TBF_STATE_H

#include <stdint.h>

#define TBF_MOVE_SEGS 8

/* one per-instance array (or its place in a packed record): instance i's part is
 * [base + i * stride, + bytes) on each side */
typedef struct tbf_move_seg {
	const unsigned char* src;
	unsigned char*       dst;
	uint64_t             srcStride, dstStride; /* bytes between instances */
	uint64_t             bytes;                /* per instance */
	uint32_t             wide;                 /* 1: 16-B loads and stores, 0: 8-B */
	uint32_t             slice0;               /* first grid slice of the segment (set by the launcher) */
} tbf_move_seg;

typedef struct tbf_move_table {
	tbf_move_seg seg[TBF_MOVE_SEGS];
	uint32_t     nseg;
	uint32_t     pad;
} tbf_move_table;

#endif
