/*
 * tbf_mixpre.inc -- the body of k_mixpre, compiled twice by tbf_render.hip:
 *   MP_KERNEL k_mixpre,     MP_EXT 0: the mixdown's gain chases and the preamp, fed from mid0
 *   MP_KERNEL k_mixpre_ext, MP_EXT 1: the preamp alone, fed from the caller's rows
 * (two plain kernels rather than a template: as a template's instantiation k_mixpre is
 * allocated two VGPRs fewer and scheduled differently, and existing kernels stay as they are).
 * The description of the chain block is above k_mixpre in tbf_render.hip.
 */
__global__ void __launch_bounds__ (MP_THREADS)
MP_KERNEL (const tbf_launch P, const tbf_seg_ctl* __restrict__ ctl)
{
	constexpr bool EXT = MP_EXT != 0;
	__shared__ MixPreLds sm;
	static_assert (sizeof (MixPreLds) <= 160 * 1024, "k_mixpre / k_mixpre_ext LDS");
	const int      w = __builtin_amdgcn_readfirstlane (threadIdx.x >> 6), lane = threadIdx.x & (NL - 1);
	const uint32_t inst0 = P.instBase + blockIdx.x * MP_CB;
	if (inst0 >= P.nInst)
		return;
	const int  nj  = (int)min ((uint32_t)MP_CB, P.nInst - inst0);
	const int  nT  = (int)P.nBlocks * MP_TPB;
	const int  nIt = nT + 3;
	const bool pre = EXT || P.chain != TBF_CHAIN_TONEGEN; /* tonegen only: no preamp */
	/* tonegen only: instances whose output k_tonegen wrote (fixed-point chases, mixFixed);
	 * a workgroup of only those has nothing to do (their state does not change) */
	if constexpr (!EXT)
		if (!pre && __all (lane >= nj || P.mixFixed[inst0 + (lane < nj ? lane : 0)]))
			return;
	if (w == 0) {
		const int      cl = min (lane, MP_ROWS - 1); /* chain row (lanes past 2 MP_CB: the idle row) */
		const int      j = min (lane >> 1, MP_CB - 1), q = lane & 1;
		const bool     ok   = lane < 2 * MP_CB && j < nj;
		tbf_mo_state*  M    = &P.st[inst0 + (ok ? j : 0)].mo;
		float          v    = 0.f;
		if constexpr (!EXT)
			v = q ? M->percEnvGain : M->keyCompLevel;
		double         iir  = q ? M->iirB : M->iirA;
		/* chase step v = v m + a: keyCompLevel + delta is (v 1) + delta, percEnvGain * decay is
		 * (v decay) + 0 (or (v 1) + 0 without percussion), the same values (v >= +0) */
		float  m = 1.f, a = 0.f, rsv = 0.f;
		bool   rs = false, hp = false;
		double ia = 0.0;
		__syncthreads ();
#if MP_PROF
		unsigned long long sw0 = 0, sb0 = 0;
#endif
#pragma unroll 1
		for (int it = 0; it < nIt; it++) {
#if MP_PROF
			const unsigned long long _s0 = __builtin_amdgcn_s_memtime ();
#endif
			if (!EXT && it < nT) {
				if (it % MP_TPB == 0) {
					const MpCtl& C = sm.c[(it / MP_TPB) % MP_CR][j];
					m   = q ? ((C.flags & MPF_PERC) ? C.decay : 1.f) : 1.f;
					a   = q ? 0.f : (C.keyCompTarget - v) / (float)TBF_BLK; /* keyCompDelta at the block start */
					rs  = q && (C.flags & MPF_RST);
					rsv = C.reset;
				}
				float* row = sm.g[it & 1][cl];
				if (__all ((v * m) + a == v)) { /* a fixed point on every lane (no percussion, the key
				                                  * compression settled): the whole tile is v */
#pragma unroll 8
					for (int k = 0; k < MP_T; k++)
						row[k] = v;
				} else {
					PRIO_UP ();
					for (int i0 = 0; i0 < MP_T; i0 += 8) {
						float o[8];
#pragma unroll
						for (int k = 0; k < 8; k++) {
							o[k] = v;
							v    = (v * m) + a;
						}
#pragma unroll
						for (int k = 0; k < 8; k++)
							row[i0 + k] = o[k];
					}
					PRIO_DOWN ();
				}
				if (it % MP_TPB == MP_TPB - 1 && rs)
					v = rsv;
			}
			const int th = it - 2; /* the high-pass (src/overdrive.cpp:104-115) of tile th */
			if (pre && th >= 0 && th < nT) {
				if (th % MP_TPB == 0) {
					const MpCtl& C = sm.c[(th / MP_TPB) % MP_CR][j];
					hp             = !(C.flags & MPF_CLEAN);
					ia             = C.iir;
				}
				if (hp) {
					const double* xr = sm.x[th % MP_XR][cl];
					double*       hr = sm.h[th & 1][cl];
					const double  om = 1.0 - ia;
					PRIO_UP ();
#pragma unroll
					for (int i0 = 0; i0 < MP_T / 2; i0 += 8) {
						double xv[8];
#pragma unroll
						for (int k = 0; k < 8; k++)
							xv[k] = xr[i0 + k];
#pragma unroll
						for (int k = 0; k < 8; k++) {
							iir        = (iir * om) + (xv[k] * ia);
							hr[i0 + k] = xv[k] - iir;
						}
					}
					PRIO_DOWN ();
				}
			}
#if MP_PROF
			const unsigned long long _s1 = __builtin_amdgcn_s_memtime ();
			sw0 += _s1 - _s0;
#endif
			__syncthreads ();
#if MP_PROF
			sb0 += __builtin_amdgcn_s_memtime () - _s1;
#endif
		}
#if MP_PROF
		if (blockIdx.x == 0 && lane == 0) {
			P.outL[P.outOffset + 8] = (float)(sw0 * 1e-3);
			P.outL[P.outOffset + 9] = (float)(sb0 * 1e-3);
			P.outL[P.outOffset + 10] = (float)((__builtin_amdgcn_s_getreg ((31 << 11) | 4) >> 4) & 3);
		}
#endif
		if (ok) {
			if (q) {
				if constexpr (!EXT)
					M->percEnvGain = v;
				M->iirB = iir;
			} else {
				if constexpr (!EXT)
					M->keyCompLevel = v;
				M->iirA = iir;
			}
		}
		return;
	}
	if (w == 1) {
		/* the control staging (block b into slot b mod MP_CR at iteration MP_TPB b - 1, from
		 * registers loaded a block earlier) and the dither stream: it advances once per sample of every
		 * block the preamp runs (src/overdrive.cpp:153-159), f[n] = the state before sample
		 * n's step */
		const bool     ok   = lane < nj;
		const uint32_t inst = inst0 + (ok ? lane : 0);
		tbf_mo_state*  M    = &P.st[inst].mo;
		uint32_t       fs   = M->odFpd;
		const int      nB   = (int)P.nBlocks;
		MpCtl          nxt;
		if (lane < MP_CB) {
			sm.c[0][lane] = mp_ctl (ctl_of (P, ctl, 0, inst));
			nxt           = mp_ctl (ctl_of (P, ctl, (uint32_t)min (1, nB - 1), inst));
		}
		bool adv = false;
		__syncthreads ();
#if MP_PROF
		unsigned long long dw0 = 0, db0 = 0;
#endif
#pragma unroll 1
		for (int it = 0; it < nIt; it++) {
#if MP_PROF
			const unsigned long long _d0 = __builtin_amdgcn_s_memtime ();
#endif
			if (lane < MP_CB) {
				if (pre && it < nT) {
					if (it % MP_TPB == 0)
						adv =!(sm.c[(it / MP_TPB) % MP_CR][lane].flags & MPF_CLEAN);
					uint32_t* f = sm.f[it & 3][lane];
#pragma unroll 8
					for (int n = 0; n < MP_T; n++) {
						f[n] = fs;
						fs   = adv ? xs_step (fs) : fs;
					}
					f[MP_T] = fs;
				}
				const int b = (it + 1) / MP_TPB; /* the block starting at the next iteration */
				if ((it + 1) % MP_TPB == 0 && b < nB) {
					sm.c[b % MP_CR][lane] = nxt;
					nxt               = mp_ctl (ctl_of (P, ctl, (uint32_t)min (b + 1, nB - 1), inst));
				}
			}
#if MP_PROF
			const unsigned long long _d1 = __builtin_amdgcn_s_memtime ();
			dw0 += _d1 - _d0;
#endif
			__syncthreads ();
#if MP_PROF
			db0 += __builtin_amdgcn_s_memtime () - _d1;
#endif
		}
#if MP_PROF
		if (blockIdx.x == 0 && lane == 0) {
			P.outL[P.outOffset + 16] = (float)(dw0 * 1e-3);
			P.outL[P.outOffset + 17] = (float)(db0 * 1e-3);
			P.outL[P.outOffset + 18] = (float)((__builtin_amdgcn_s_getreg ((31 << 11) | 4) >> 4) & 3);
		}
#endif
		if (ok && pre && lane < MP_CB)
			M->odFpd = fs;
		return;
	}
	/* helpers: task t = instance h + MP_H t, lane n = sample n of the tile.
	 * The (s, p) input is read two iterations before its use, into two register sets
	 * alternating by iteration parity (the loop is unrolled by two, so the sets stay static) */
	const int     h = w - 2, n = lane & (MP_T - 1);
	using In = typename std::conditional<EXT, float, float2>::type; /* a sample of the stage's input */
	const In*     in[MP_NTK];
	float*        o1[MP_NTK];
	float*        oL[MP_NTK];
	float*        oR[MP_NTK];
	int           jT[MP_NTK], rT[MP_NTK];
	bool          okT[MP_NTK];
	In            pS[2][MP_NTK];
#pragma unroll
	for (int t = 0; t < MP_NTK; t++) {
		const int j       = h + MP_H * t;
		okT[t]            = j < nj;
		jT[t]             = okT[t] ? j : nj - 1;
		const uint32_t is = inst0 + jT[t];
		if constexpr (EXT)
			in[t] = (const In*)P.ext + (size_t)is * P.extStride + P.extOffset + n;
		else
			in[t] = (const In*)P.mid0 + (size_t)is * P.midStride + n;
		o1[t]             = P.mid1 ? P.mid1 + (size_t)is * P.midStride + n : nullptr;
		oL[t]             = P.outL + (size_t)is * P.outStride + P.outOffset + n;
		oR[t]             = P.outR + (size_t)is * P.outStride + P.outOffset + n;
		/* sample n's high-pass chain: iirSampleA takes the samples of parity 0 when fpFlip
		 * is set at the block start (128 samples leave it unchanged), else parity 1 */
		const int q0      = P.st[is].mo.fpFlip ? 0 : 1;
		rT[t]             = 2 * jT[t] + ((n & 1) ^ q0);
		pS[0][t]          = in[t][0];
		pS[1][t]          = in[t][(size_t)min (1, nT - 1) * MP_T];
	}
	const bool tap = P.chain == TBF_CHAIN_TAP_PREAMP;
#if MP_PROF /* profiling variant only: s_memtime per helper section, written over instance 0's output */
	unsigned long long pf[3] = {0, 0, 0};
#define MP_T0() const unsigned long long _t0 = __builtin_amdgcn_s_memtime ()
#define MP_TS(i, a) { asm volatile ("" ::: "memory"); const unsigned long long _t = __builtin_amdgcn_s_memtime (); pf[i] += _t - (a); }
#else
#define MP_T0()
#define MP_TS(i, a)
#endif
	__syncthreads ();
	auto step = [&] (const int it, In (&qS)[MP_NTK]) {
		MP_T0 ();
		/* the waveshaper of tile it - 3: high-pass output, dry input, the dither state after
		 * the sample's step */
		const int kw = it - 3;
		if (pre && kw >= 0 && kw < nT) {
			const size_t so = (size_t)kw * MP_T;
#if MP_NTK > 1
			/* the tasks' waveshapers side by side (preamp_shape_n) */
			float ys[MP_NTK];
			{
				const MpCtl* Cp[MP_NTK];
				double       xd[MP_NTK], xh[MP_NTK];
				uint32_t     f1[MP_NTK];
				bool         cl[MP_NTK];
				bool         allCl = true;
#pragma unroll
				for (int t = 0; t < MP_NTK; t++) {
					Cp[t] = &sm.c[(kw / MP_TPB) % MP_CR][jT[t]];
					xd[t] = sm.x[kw % MP_XR][rT[t]][n >> 1];
					xh[t] = sm.h[kw & 1][rT[t]][n >> 1];
					f1[t] = sm.f[kw & 3][jT[t]][n + 1];
					cl[t] = (Cp[t]->flags & MPF_CLEAN) != 0;
					allCl = allCl && cl[t];
				}
				if (!__all (allCl))
					preamp_shape_n<MP_NTK> (xh, xd, Cp, f1, ys);
#pragma unroll
				for (int t = 0; t < MP_NTK; t++)
					if (cl[t])
						ys[t] = (float)xd[t];
			}
#endif
#pragma unroll
			for (int t = 0; t < MP_NTK; t++) {
#if MP_NTK > 1
				const float y = ys[t];
#else
				const MpCtl& C  = sm.c[(kw / MP_TPB) % MP_CR][jT[t]];
				const double xd = sm.x[kw % MP_XR][rT[t]][n >> 1];
				float        y;
				if (C.flags & MPF_CLEAN)
					y = (float)xd;
				else
					y = preamp_shape (sm.h[kw & 1][rT[t]][n >> 1], xd, C, sm.f[kw & 3][jT[t]][n + 1]);
#endif
				if (okT[t]) {
					if (tap) {
						oL[t][so] = y;
						oR[t][so] = y;
					} else
						o1[t][so] = y;
				}
			}
		}
#if MP_PROF
		const unsigned long long _t1 = __builtin_amdgcn_s_memtime ();
		pf[0] += _t1 - _t0;
#endif
		/* the products of tile it - 1 (src/tonegen.cpp:3734-3777) and the preamp input:
		 * denormal guard with the dither state before the sample (src/overdrive.cpp:95-100) */
		const int kp = it - 1;
		if (kp >= 0 && kp < nT) {
#pragma unroll
			for (int t = 0; t < MP_NTK; t++) {
				const MpCtl& C  = sm.c[(kp / MP_TPB) % MP_CR][jT[t]];
#if MP_EXT
				const float  y  = qS[t]; /* the caller's sample is the preamp input */
#else
				const float  kc = sm.g[kp & 1][2 * jT[t]][n];
				const float  pe = sm.g[kp & 1][2 * jT[t] + 1][n];
				const float2 sp = qS[t];
				const float  y  = (C.flags & MPF_PERC) ? (C.gain * kc * (sp.x + (sp.y * pe))) : (C.gain * kc * sp.x);
#endif
				if (!pre) {
					if (okT[t] && !P.mixFixed[inst0 + jT[t]]) {
						oL[t][(size_t)kp * MP_T] = y;
						oR[t][(size_t)kp * MP_T] = y;
					}
				} else {
					double x = (double)y;
					if (!(C.flags & MPF_CLEAN) && fabs (x) < 1.18e-23)
						x = sm.f[kp & 3][jT[t]][n] * 1.18e-17;
					sm.x[kp % MP_XR][rT[t]][n >> 1] = x;
				}
			}
		}
		/* the input of tile it + 1 into the set just consumed (clamped past the last tile: a
		 * harmless re-read, so the loads need no branch) */
		const int tl = min (it + 1, nT - 1);
#pragma unroll
		for (int t = 0; t < MP_NTK; t++)
			qS[t] = in[t][(size_t)tl * MP_T];
#if MP_PROF
		const unsigned long long _t2 = __builtin_amdgcn_s_memtime ();
		pf[1] += _t2 - _t1;
#endif
		__syncthreads ();
		MP_TS (2, _t2);
	};
#pragma unroll 1
	for (int it = 0; it < nIt; it += 2) {
		step (it, pS[1]);
		if (it + 1 < nIt)
			step (it + 1, pS[0]);
	}
#if MP_PROF
	if (blockIdx.x == 0 && h == 0 && lane == 0)
		for (int i = 0; i < 3; i++)
			P.outL[P.outOffset + i] = (float)(pf[i] * 1e-3);
	if (blockIdx.x == 0 && lane == 0) { /* every helper: its sections and its SIMD (HW_ID bits 5:4) */
		for (int i = 0; i < 3; i++)
			P.outL[P.outOffset + 32 + 4 * h + i] = (float)(pf[i] * 1e-3);
		P.outL[P.outOffset + 32 + 4 * h + 3] = (float)((__builtin_amdgcn_s_getreg ((31 << 11) | 4) >> 4) & 3);
	}
#endif
#undef MP_T0
#undef MP_TS
}
