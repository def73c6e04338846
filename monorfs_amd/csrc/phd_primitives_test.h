// phd_primitives_test.h — test surface (phd_test_primitive): the small __device__ functions of phd_device.h, phd_resample.h,
// phd_alpha.h and phd_prune.h, each called on records handed in by the host, so that a test can hold the source function — its
// constants, pragmas, inline assembly and order of operations — to a reference of its own (tests/primitive_cases.py). No step
// kernel calls anything in here. A primitive inlined into this kernel need not compile to the instructions it has inside
// k_sweep; what is pinned is the source text the two share ("Device primitives").
//
// Inputs and outputs are raw bytes: NaN payloads, -0.0 and 64-bit patterns pass unchanged. f64 = double, u64 / i64 / i32 =
// integers, all little-endian, records packed without padding. `n` is the number of records. Workgroups of 256 threads but
// for PT_BLOCK_SUM_512 / _1024. The ops whose functions talk across a wave or a workgroup take whole workgroups only (n a
// multiple of the workgroup size; thread t of workgroup b holds record 256 b + t): every lane is live, as in their callers.
//
//   op                    in (per record; [head] once in front)           out (per record)
//   PT_EXP_NEG            f64 x                                           f64 exp_neg(x, T)
//   PT_EXP_TAB            (nothing; n = 256)                              f64 T[j] as exp_tab_init left it in LDS
//   PT_EXP_PAIR           f64 x, u64 keep (0 / 1)                         f64 exp_pair(x, T, keep)
//   PT_GAUSS_RECORD       f64 w, m[3], Pi[6], mult                        f64 g[10]
//   PT_GAUSS_LOGW         f64 g[10], x[3]                                 f64 l = gauss_logw(g, x - g[0..2]), exp_pair(l, T)
//   PT_DD_TWO_SUM         f64 a, b                                        f64 hi, lo
//   PT_DD_QUICK           f64 a, b (|a| >= |b|)                           f64 hi, lo
//   PT_DD_TWO_SUM_PROD    f64 a, b, c                                     f64 hi, lo of dd_two_sum(a * b, c): the product is formed HERE,
//                                                                          where contraction is on; only the helper's own pragma keeps
//                                                                          its first addition from fusing with it
//   PT_DD_ADD             f64 x.hi, x.lo, y.hi, y.lo                      f64 hi, lo
//   PT_DD_ADD_D           f64 x.hi, x.lo, d                               f64 hi, lo
//   PT_DD_SCAN_64 / _16   f64 hi, lo (a lane)                             f64 hi, lo of dd_wave_scan(v, lane, 64 / 16)
//   PT_SLOT_TARGET        i64 i, f64 R0, invP                             f64 hi, lo
//   PT_SMALL_DIV          i32 d (1 <= d < 2^24)                           u64 count of s in [0, 2^24) with small_div(s, d, 1.0f / d)
//                                                                          != s / d, u64 2^24 - (the first such s) (0: none)
//   PT_BIN_OF_BITS        [f64 MinWeight] u64 bits                        i32 weight_bin_of_bits(bits, weight_bin_base(MinWeight))
//   PT_BIN_OF_KEY         [f64 MinWeight] f64 w                           i32 weight_bin_of_bits(prune_key(w), base)
//   PT_BIN_EDGE           [f64 MinWeight] (n = 1024)                      u64 out[0] = base, out[b] = bits of weight_bin_edge(b, base)
//   PT_WAVE_SUM / _MAX / _MIN   f64 v (a lane)                            f64 the lane's result
//   PT_WAVE_INCL_SCAN     i32 v (a lane)                                  i32 the lane's result
//   PT_WAVE_FIRST_MAX     f64 v, u64 has (a lane)                         f64 m, i64 the lane returned
//   PT_BLOCK_SUM_256T / _512 / _1024   f64 v (a thread; workgroups of 256 / 512 / 1024)   f64 block_sum_1024(v, scratch, tid)
//   PT_BLOCK_SUM_256      f64 s4[4]                                       f64 block_sum_256(s4)
//   PT_BLOCK_TREE_SUM     f64 v (a thread)                                f64 block_tree_sum(red, v, tid)
//   PT_INV_SYM3           f64 P[6]                                        f64 inv[6], det
//   PT_INV_GEN3           f64 a[9]                                        f64 inv[9], det
//   PT_QUAD_SYM           f64 A[6], d[3]                                  f64 quad_sym(A, d)
//   PT_QUAD_GEN           f64 A[9], d[3]                                  f64 quad_gen(A, d)
#pragma once
#include "phd_device.h"
#include "phd_resample.h"
#include "phd_prune.h"
#include "phd_alpha.h"

enum {
	PT_EXP_NEG = 1, PT_EXP_TAB, PT_EXP_PAIR, PT_GAUSS_RECORD, PT_GAUSS_LOGW,
	PT_DD_TWO_SUM, PT_DD_QUICK, PT_DD_TWO_SUM_PROD, PT_DD_ADD, PT_DD_ADD_D, PT_DD_SCAN_64, PT_DD_SCAN_16, PT_SLOT_TARGET,
	PT_SMALL_DIV, PT_BIN_OF_BITS, PT_BIN_OF_KEY, PT_BIN_EDGE,
	PT_WAVE_SUM, PT_WAVE_MAX, PT_WAVE_MIN, PT_WAVE_INCL_SCAN, PT_WAVE_FIRST_MAX,
	PT_BLOCK_SUM_256T, PT_BLOCK_SUM_512, PT_BLOCK_SUM_1024, PT_BLOCK_SUM_256, PT_BLOCK_TREE_SUM,
	PT_INV_SYM3, PT_INV_GEN3, PT_QUAD_SYM, PT_QUAD_GEN, PT_OPS_END
};

#define PT_SMALL_DIV_RANGE (1 << 24)   // the sweep of PT_SMALL_DIV: every s below it
#define PT_SMALL_DIV_PER_THREAD 64     // ... a thread takes this many, a stride of 256 apart
#define PT_MAX_RECORDS (1 << 22)
#define PT_LDS_DOUBLES (EXPTAB_N + 256 + 16)

// The layout of an op: bytes of the head, of an input and an output record, threads of a workgroup, whether n must fill
// whole workgroups, and a fixed n (0: from the input's size). false: no such op.
struct PrimLayout { int head, in_rec, out_rec, block; bool whole; int fixed_n; };
inline bool primitive_layout(int op, PrimLayout& l)
{
	switch (op) {
	case PT_EXP_NEG:         l = {0, 8, 8, 256, false, 0}; return true;
	case PT_EXP_TAB:         l = {0, 0, 8, 256, false, EXPTAB_N}; return true;
	case PT_EXP_PAIR:        l = {0, 16, 8, 256, false, 0}; return true;
	case PT_GAUSS_RECORD:    l = {0, 88, 80, 256, false, 0}; return true;
	case PT_GAUSS_LOGW:      l = {0, 104, 16, 256, false, 0}; return true;
	case PT_DD_TWO_SUM:
	case PT_DD_QUICK:        l = {0, 16, 16, 256, false, 0}; return true;
	case PT_DD_TWO_SUM_PROD: l = {0, 24, 16, 256, false, 0}; return true;
	case PT_DD_ADD:          l = {0, 32, 16, 256, false, 0}; return true;
	case PT_DD_ADD_D:        l = {0, 24, 16, 256, false, 0}; return true;
	case PT_DD_SCAN_64:
	case PT_DD_SCAN_16:      l = {0, 16, 16, 256, true, 0}; return true;
	case PT_SLOT_TARGET:     l = {0, 24, 16, 256, false, 0}; return true;
	case PT_SMALL_DIV:       l = {0, 4, 16, 256, false, 0}; return true;
	case PT_BIN_OF_BITS:
	case PT_BIN_OF_KEY:      l = {8, 8, 4, 256, false, 0}; return true;
	case PT_BIN_EDGE:        l = {8, 0, 8, 256, false, 1024}; return true;
	case PT_WAVE_SUM:
	case PT_WAVE_MAX:
	case PT_WAVE_MIN:        l = {0, 8, 8, 256, true, 0}; return true;
	case PT_WAVE_INCL_SCAN:  l = {0, 4, 4, 256, true, 0}; return true;
	case PT_WAVE_FIRST_MAX:  l = {0, 16, 16, 256, true, 0}; return true;
	case PT_BLOCK_SUM_256T:  l = {0, 8, 8, 256, true, 0}; return true;
	case PT_BLOCK_SUM_512:   l = {0, 8, 8, 512, true, 0}; return true;
	case PT_BLOCK_SUM_1024:  l = {0, 8, 8, 1024, true, 0}; return true;
	case PT_BLOCK_SUM_256:   l = {0, 32, 8, 256, false, 0}; return true;
	case PT_BLOCK_TREE_SUM:  l = {0, 8, 8, 256, true, 0}; return true;
	case PT_INV_SYM3:        l = {0, 48, 56, 256, false, 0}; return true;
	case PT_INV_GEN3:        l = {0, 72, 80, 256, false, 0}; return true;
	case PT_QUAD_SYM:        l = {0, 72, 8, 256, false, 0}; return true;
	case PT_QUAD_GEN:        l = {0, 96, 8, 256, false, 0}; return true;
	}
	return false;
}

// `in` points at the head (if the op has one), the records follow it; `out` is zero when the kernel starts. PT_SMALL_DIV runs
// a grid of (PT_SMALL_DIV_RANGE / (256 * PT_SMALL_DIV_PER_THREAD), n) workgroups, every other op ceil(n / blockDim.x).
__global__ __launch_bounds__(1024) void k_test_primitive(int op, const char* __restrict__ in, char* __restrict__ out, int n)
{
	extern __shared__ double pt_lds[];   // PT_LDS_DOUBLES of them, from the launch: the exponential's table, block_tree_sum's red[256], block_sum_1024's scratch
	double* const etab = pt_lds;
	double* const red = pt_lds + EXPTAB_N;
	double* const s16 = red + 256;
	const int tid = threadIdx.x, lane = tid & 63;
	const int i = blockIdx.x * blockDim.x + tid;
	const bool live = i < n;
	exp_tab_init(etab, tid);
	__syncthreads();
	const double* const fin = (const double*) in;
	double* const fout = (double*) out;
	switch (op) {
	case PT_EXP_NEG:
		if (live) fout[i] = exp_neg(fin[i], etab);
		break;
	case PT_EXP_TAB:
		if (live) fout[i] = etab[i];
		break;
	case PT_EXP_PAIR:
		if (live) fout[i] = exp_pair(fin[2 * i], etab, ((const unsigned long long*) in)[2 * i + 1] != 0);
		break;
	case PT_GAUSS_RECORD:
		if (live) {
			const double* r = fin + (size_t) i * 11;
			const double m[3] = {r[1], r[2], r[3]}, Pi[6] = {r[4], r[5], r[6], r[7], r[8], r[9]};
			double g[10];
			gauss_record(r[0], m, Pi, r[10], g);
			for (int t = 0; t < 10; t++) fout[(size_t) i * 10 + t] = g[t];
		}
		break;
	case PT_GAUSS_LOGW:
		if (live) {
			const double* g = fin + (size_t) i * 13;
			const double l = gauss_logw(g, g[10] - g[0], g[11] - g[1], g[12] - g[2]);
			fout[2 * i] = l;
			fout[2 * i + 1] = exp_pair(l, etab);
		}
		break;
	case PT_DD_TWO_SUM:
	case PT_DD_QUICK:
		if (live) {
			const dd r = (op == PT_DD_TWO_SUM) ? dd_two_sum(fin[2 * i], fin[2 * i + 1]) : dd_quick(fin[2 * i], fin[2 * i + 1]);
			fout[2 * i] = r.hi; fout[2 * i + 1] = r.lo;
		}
		break;
	case PT_DD_TWO_SUM_PROD:
		if (live) {
			const dd r = dd_two_sum(fin[3 * i] * fin[3 * i + 1], fin[3 * i + 2]);
			fout[2 * i] = r.hi; fout[2 * i + 1] = r.lo;
		}
		break;
	case PT_DD_ADD:
		if (live) {
			const dd r = dd_add(dd{fin[4 * i], fin[4 * i + 1]}, dd{fin[4 * i + 2], fin[4 * i + 3]});
			fout[2 * i] = r.hi; fout[2 * i + 1] = r.lo;
		}
		break;
	case PT_DD_ADD_D:
		if (live) {
			const dd r = dd_add_d(dd{fin[3 * i], fin[3 * i + 1]}, fin[3 * i + 2]);
			fout[2 * i] = r.hi; fout[2 * i + 1] = r.lo;
		}
		break;
	case PT_DD_SCAN_64:
	case PT_DD_SCAN_16: {
		const dd v = {fin[2 * i], fin[2 * i + 1]};
		const dd r = (op == PT_DD_SCAN_64) ? dd_wave_scan(v, lane) : dd_wave_scan(v, lane, 16);
		fout[2 * i] = r.hi; fout[2 * i + 1] = r.lo;
		break;
	}
	case PT_SLOT_TARGET:
		if (live) {
			const dd r = slot_target((int) ((const long long*) in)[3 * i], fin[3 * i + 1], fin[3 * i + 2]);
			fout[2 * i] = r.hi; fout[2 * i + 1] = r.lo;
		}
		break;
	case PT_SMALL_DIV: {
		const int d = ((const int*) in)[blockIdx.y];
		const float rd = 1.0f / (float) d;
		const int s0 = blockIdx.x * (256 * PT_SMALL_DIV_PER_THREAD) + tid;
		unsigned int bad = 0, first = 0;
		for (int t = 0; t < PT_SMALL_DIV_PER_THREAD; t++) {
			const int s = s0 + 256 * t;
			if (small_div(s, d, rd) != s / d) { bad++; first = max(first, (unsigned int) (PT_SMALL_DIV_RANGE - s)); }
		}
		unsigned long long* o = (unsigned long long*) out + 2 * (size_t) blockIdx.y;
		if (bad) { atomicAdd(o, (unsigned long long) bad); atomicMax(o + 1, (unsigned long long) first); }
		break;
	}
	case PT_BIN_OF_BITS:
		if (live) ((int*) out)[i] = weight_bin_of_bits(((const unsigned long long*) in)[1 + i], weight_bin_base(fin[0]));
		break;
	case PT_BIN_OF_KEY:
		if (live) ((int*) out)[i] = weight_bin_of_bits(prune_key(fin[1 + i]), weight_bin_base(fin[0]));
		break;
	case PT_BIN_EDGE:
		if (live) {
			const unsigned int base = weight_bin_base(fin[0]);
			((unsigned long long*) out)[i] = (i == 0) ? (unsigned long long) base : (unsigned long long) __double_as_longlong(weight_bin_edge(i, base));
		}
		break;
	case PT_WAVE_SUM: fout[i] = wave_sum(fin[i]); break;
	case PT_WAVE_MAX: fout[i] = wave_max(fin[i]); break;
	case PT_WAVE_MIN: fout[i] = wave_min(fin[i]); break;
	case PT_WAVE_INCL_SCAN: ((int*) out)[i] = wave_incl_scan(((const int*) in)[i]); break;
	case PT_WAVE_FIRST_MAX: {
		double m;
		const int l = wave_first_max(fin[2 * i], ((const unsigned long long*) in)[2 * i + 1] != 0, m);
		fout[2 * i] = m; ((long long*) out)[2 * i + 1] = l;
		break;
	}
	case PT_BLOCK_SUM_256T:
	case PT_BLOCK_SUM_512:
	case PT_BLOCK_SUM_1024: fout[i] = block_sum_1024(fin[i], s16, tid); break;
	case PT_BLOCK_SUM_256:
		if (live) fout[i] = block_sum_256(fin + 4 * (size_t) i);
		break;
	case PT_BLOCK_TREE_SUM: fout[i] = block_tree_sum(red, fin[i], tid); break;
	case PT_INV_SYM3:
		if (live) {
			const double* r = fin + (size_t) i * 6;
			const double P[6] = {r[0], r[1], r[2], r[3], r[4], r[5]};
			double inv[6], det;
			inv_sym3(P, inv, det);
			for (int t = 0; t < 6; t++) fout[(size_t) i * 7 + t] = inv[t];
			fout[(size_t) i * 7 + 6] = det;
		}
		break;
	case PT_INV_GEN3:
		if (live) {
			double a[9], inv[9], det;
			for (int t = 0; t < 9; t++) a[t] = fin[(size_t) i * 9 + t];
			inv_gen3(a, inv, det);
			for (int t = 0; t < 9; t++) fout[(size_t) i * 10 + t] = inv[t];
			fout[(size_t) i * 10 + 9] = det;
		}
		break;
	case PT_QUAD_SYM:
		if (live) {
			const double* r = fin + (size_t) i * 9;
			const double A[6] = {r[0], r[1], r[2], r[3], r[4], r[5]};
			fout[i] = quad_sym(A, r[6], r[7], r[8]);
		}
		break;
	case PT_QUAD_GEN:
		if (live) {
			double A[9];
			for (int t = 0; t < 9; t++) A[t] = fin[(size_t) i * 12 + t];
			fout[i] = quad_gen(A, fin[(size_t) i * 12 + 9], fin[(size_t) i * 12 + 10], fin[(size_t) i * 12 + 11]);
		}
		break;
	}
}
