// phd_prune.h — k_prune_merge: PruneModel (PHDNavigator.cs:913-948) for one particle per workgroup.
//
// The reference sorts the corrected mixture by weight, keeps the first min(MaxQuantity, #w >= MinWeight)
// entries and then, in weight order, lets every still-present entry i absorb every later entry k with
// (m_i - m_k)^T P_i^-1 (m_i - m_k) < MergeThreshold^2 (Gaussian.AreClose, Gaussian.cs:243-246), replacing
// the set by its moment match (Gaussian.Merge, Gaussian.cs:297-347).
//
// Only the question "is i still present" is sequential. prune_merge_body (one workgroup, one particle; inside k_prune_merge,
// k_emit_prune and k_particle_chain) therefore splits the work into five phases, each behind a workgroup barrier. Its LDS pool has one
// statement, PruneLds / prune_lds / prune_pool below: the sort half and the ranked ordering's arrays of phase A share their place with
// the merge half of phases B - D. A, S, C and B's grid are functions; B's two walks and D are blocks of the body (as functions they cost
// k_prune_merge three registers — DESIGN.md); the parts they share are the small prune_* functions in front of phase A.
//   A. order    : prune_order. A histogram over the weights' leading bits finds the bin of the cut-th heaviest entry; the entries
//                 from that bin up are ranked inside their bins (a counting sort, no sorting network). When they do not fit: a
//                 bitonic sort on the weight's bit pattern (one 32-bit word per entry: key + emit slot), held in
//                 registers (thread exchanges, lane shuffles, LDS only for the longest distances), the best
//                 half kept while further chunks stream in; runs of equal keys are then put in (weight,
//                 canonical index) order, which makes the order the reference's sort made stable
//   S. stage    : prune_gather. The kept records are gathered once, in sorted order, into a slab of 96-byte rows in HBM (the
//                 component record, as the banks and the emitted list hold it, + its canonical index: a gathered row
//                 is two 64-byte sectors whatever its origin, a row read back is one or two lines); the Euclidean
//                 bounds go to LDS, the means of a thread's rows stay in its registers for the grid
//   B. pairs    : every closeness test close_i(k), k > i, in parallel, one row per thread. A Euclidean bound
//                 |d|^2 > T^2 trace(P_i)  =>  d^T P_i^-1 d >= |d|^2 / lambda_max(P_i) > T^2
//                 limits the candidates of a row to a ball; the rows are binned in a uniform grid (hashed
//                 cells) and the <= 8 buckets the ball meets are walked as one list of float32 records, the
//                 survivors of the float32 distance test take the exact FP64 test. Each row keeps its first 7
//                 close rows. The rows go to the lanes in the order of their candidate counts (a second counting
//                 sort), so that a wave is not held up by the one row of a crowded cell in it.
//   C. resolve  : one wave walks the rows in weight order, 64 row records at a time held in its lanes and
//                 the "absorbed" bits spread over its lanes (integer work only); rows with more than 7
//                 close rows are re-tested by the 64 lanes.
//   D. merge    : one thread per surviving row accumulates the raw moments of its set in list order
//                 (leader first, members by rank — the reference's summation order) and writes the
//                 result at its position among the survivors.
#pragma once
#include "phd_device.h"

#define PRUNE_NBR 7
#ifndef PRUNE_NB
#define PRUNE_NB 2048   // buckets of the spatial hash (16-bit counters, two per LDS word; 4096 until round 4: half of them, and the bounds below as
#endif                  // float32, take MaxQuantity 1024's working set from 58.7 to 50.5 KB — three workgroups per CU instead of two on config S)
#ifndef PRUNE_HEAVY
#define PRUNE_HEAVY 32  // a row with more candidates than this is searched by a whole wave
#endif
#define PRUNE_ROW 12    // doubles per row of the sorted slab: w, m[3], P[6] (a component record), canonical index, spare

// The LDS pool of the body, stated once: prune_lds() lays it out (offsets in 4-byte words from the pool's start), prune_pool() turns
// the offsets into pointers, and every total is derived from the arrays' own sizes. Three groups share the stretch from `x` on:
//   sort half    sw | w2                                            phase A's sorting passes; the gather reads sw
//   ranked       kw | ks over sw | w2, hist | out | ki behind them   phase A's ranked ordering (it never writes sw | w2); the gather reads
//                                                                   out, kw, ks, ki
//   merge half   nbr | cand | owner | cw | absb | ord | rowpos       over both, from the barrier that closes the gather to the end
// `rad2` in front (written by the gather, read by B) and the tail behind (`bred`: the gather's reduction, read once behind its barrier;
// `scan` over it from B's prefix on) overlay nothing else.
// The ranked arrays always fit: kw and ks take 3 capN <= 2 NS words, the sort arrays' place, since capN = (2 NS) / 3; hist, out and ki
// lie behind, and the tail starts at or behind their end — for every cutcap, since all three launches size the pool with
// prune_lds(cutcap). So the ranked ordering asks the pool nothing (scripts/probes/prune_lds_table.hip asserts it for cutcap 1 .. 6000).
struct PruneLds {
	int rad2, x, scan;       // offsets in doubles
	int NS;                  // sort width (power of two >= 2 * cutcap)
	int bytes;
	int cc, capN;            // cutcap rounded up to even; entries the ranked ordering holds (12 bytes each in the sort arrays' place)
	// offsets in 4-byte words
	int sw, w2;                                         // u32[NS] sort words (prune_pack32) | u32[NS] the 32 weight bits behind the key of slot e < NS
	int kw, ks, hist, out, ki, ranked_end;              // u64[capN] full keys, bin after bin | u32[capN] their slots | int[HIST] | u32[capN] place of rank r | u32[capN] canonical indices
	int nbr, cand, owner, cw, absb, ord, rowpos, merge_end;   // u64[cc][2] | float4[cc] | int[cc] | u32[CW] | u64[64] | u16[cc] | u16[cc]
	static constexpr int BINS = 1024;                   // weight bins of the histogram (weight_bin_of_bits)
	static constexpr int HIST = BINS + 4 + 4;           // the bins' counts (then starts, then ends) | s_T, s_cnt, s_fill, s_maxb | pad
	static constexpr int CW = (PRUNE_NB + 2) / 2 + 1;   // two 16-bit bucket boundaries per word, cstart[NB + 2] | a pad word (absb stays 8-byte aligned)
	static constexpr int ABSB = 2 * 64;                 // u64[64]
	static constexpr int RANKED_PAD = 4, MERGE_PAD = 8; // spare words behind ki and behind rowpos
	static constexpr int SCAN = 264, TAIL_PAD = 8;      // int[264] scan (over double[28] bred) | spare words
};
static_assert(PruneLds::HIST % 2 == 0 && PruneLds::CW % 2 == 0 && PruneLds::ABSB % 2 == 0 && PruneLds::RANKED_PAD % 2 == 0 && PruneLds::MERGE_PAD % 2 == 0,
              "PruneLds: every group must end on a double (scan = end / 2) and absb start on one: PRUNE_NB must be a multiple of 4");

__host__ __device__ inline PruneLds prune_lds(int cutcap)
{
	PruneLds l;
	const int cc = (cutcap + 1) & ~1;
	int NS = 512;
	while (NS < 2 * cutcap) NS <<= 1;
	l.NS    = NS;
	l.cc    = cc;
	l.capN  = (NS * 2) / 3;
	l.rad2  = 0;
	l.x     = l.rad2 + ((cc / 2 + 1) & ~1);   // rad2: float32[cc], padded to 16 bytes
	const int x = 2 * l.x;
	l.sw = x; l.w2 = l.sw + NS;
	const int sort_end = l.w2 + NS;
	l.kw = x; l.ks = l.kw + 2 * l.capN;       // (ks ends at x + 3 capN <= sort_end)
	l.hist = sort_end; l.out = l.hist + PruneLds::HIST; l.ki = l.out + l.capN;
	l.ranked_end = l.ki + l.capN + PruneLds::RANKED_PAD;
	l.nbr = x; l.cand = l.nbr + 4 * cc; l.owner = l.cand + 4 * cc; l.cw = l.owner + cc; l.absb = l.cw + PruneLds::CW;
	l.ord = l.absb + PruneLds::ABSB; l.rowpos = l.ord + cc / 2;
	l.merge_end = l.ord + 4 * (cc / 4 + 1) + PruneLds::MERGE_PAD;   // (ord and rowpos: cc words, rounded up)
	int end = sort_end;                       // the three groups' ends are all even (cc is, and the static_assert behind the struct)
	if (l.ranked_end > end) end = l.ranked_end;
	if (l.merge_end > end) end = l.merge_end;
	l.scan  = end / 2;
	l.bytes = (2 * l.scan + PruneLds::SCAN + PruneLds::TAIL_PAD) * 4;
	return l;
}

// the pool's arrays as pointers (see PruneLds for who overlays whom)
struct PrunePool {
	float* rad2;                       // [cut] squared Euclidean bound of row i (inf: none), float32 rounded UP: a sound bound stays one
	unsigned int *sw, *w2;
	unsigned long long* kw;
	unsigned int* ks;
	int* hist;                         // [BINS] bins, then s_T, s_cnt, s_fill, s_maxb
	unsigned int *out, *ki;
	unsigned long long* nbr;           // [cut][2]: count + up to 7 close later rows
	float4* cand;                      // [cut] rows grouped by bucket: mean relative to the box (float32), row
	int* owner;                        // [cut] row that absorbed k (-1: none); the row's bucket, then its candidate count, while the grid is built
	unsigned int* cw;                  // [(NB + 2) / 2] two 16-bit bucket boundaries per word
	const unsigned short* cstart;      // [NB + 2] the same as 16-bit words: bucket b is [cstart[b], cstart[b + 1])
	unsigned long long* absb;          // [64] absorbed bits as left by the resolving wave
	unsigned short *ord, *rowpos;      // [cut] rows in the order the pair search takes them | position of row r in `cand`
	int* scan;                         // [264]
	double* bred;                      // [28] block reduction scratch (before `scan` is used)
};
__device__ __forceinline__ PrunePool prune_pool(double* smem, const PruneLds& l)
{
	unsigned int* const w = (unsigned int*) smem;
	PrunePool o;
	o.rad2 = (float*) (smem + l.rad2);
	o.sw = w + l.sw; o.w2 = w + l.w2;
	o.kw = (unsigned long long*) (w + l.kw); o.ks = w + l.ks; o.hist = (int*) (w + l.hist); o.out = w + l.out; o.ki = w + l.ki;
	o.nbr = (unsigned long long*) (w + l.nbr); o.cand = (float4*) (w + l.cand); o.owner = (int*) (w + l.owner); o.cw = w + l.cw;
	o.cstart = (const unsigned short*) o.cw;
	o.absb = (unsigned long long*) (w + l.absb); o.ord = (unsigned short*) (w + l.ord); o.rowpos = (unsigned short*) (w + l.rowpos);
	o.scan = (int*) (smem + l.scan); o.bred = smem + l.scan;
	return o;
}

// total order on doubles as unsigned integers (larger double <-> larger key); 0 is below every number
__device__ __forceinline__ unsigned long long prune_key(double w)
{
	unsigned long long b = (unsigned long long) __double_as_longlong(w);
	return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// Sort entries are one 64-bit word: the top 44 bits of the weight's key (sign, exponent, 32 mantissa bits),
// then a 20-bit payload (slot). Entries whose weights agree in those 44 bits (relative difference below
// 2.4e-10) come out adjacent in arbitrary order; the caller then orders each such run by (full weight desc,
// canonical index asc) — the reference's sort made stable. 0 sorts last (padding).
#define PRUNE_SLOT_BITS 20
#define PRUNE_SLOT_MASK ((1u << PRUNE_SLOT_BITS) - 1u)
__device__ __forceinline__ unsigned long long prune_pack(double w, int slot)
{
	return (prune_key(w) & ~(unsigned long long) PRUNE_SLOT_MASK) | (unsigned int) slot;
}
__device__ __forceinline__ int prune_slot(unsigned long long v) { return (int) ((unsigned int) v & PRUNE_SLOT_MASK); }
__device__ __forceinline__ unsigned long long prune_kbits(unsigned long long v) { return v >> PRUNE_SLOT_BITS; }

template <class W>
__device__ __forceinline__ void prune_ce(W* v, int t, int j, int k)
{
	int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
	int q = i | j;
	W a = v[i], b = v[q];
	bool desc = (i & k) == 0;
	if (desc ? (a < b) : (a > b)) { v[i] = b; v[q] = a; }
}

// bitonic sort of n (power of two) words, largest first, by 256 threads. Compare-exchange t belongs to the
// 128-element block t / 64 for every distance j <= 64, and a wave keeps the same blocks from one distance to
// the next, so those sub-steps need no workgroup barrier — only the distances >= 128 and the stage ends do.
template <class W>
__device__ __forceinline__ void prune_bitonic(W* v, int n, int tid)
{
	for (int k = 2; k <= n; k <<= 1) {
		int j = k >> 1;
		for (; j >= 128; j >>= 1) {
			for (int t = tid; t < (n >> 1); t += 256) prune_ce(v, t, j, k);
			__syncthreads();
		}
		for (; j > 0; j >>= 1) {
			for (int t = tid; t < (n >> 1); t += 256) prune_ce(v, t, j, k);
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
			__builtin_amdgcn_wave_barrier();
		}
		__syncthreads();
	}
}

// In-register bitonic sort of n = 256 * EPT words, largest first: thread t holds the EPT consecutive words
// sv[t * EPT ..). Distances below EPT are exchanges inside a thread, distances below 64 * EPT are lane
// shuffles inside a wave; only the few larger ones go through LDS.
template <int EPT, class W>
__device__ __forceinline__ void prune_sort_regs(W* sv, int tid)
{
	constexpr int n = 256 * EPT;
	W v[EPT];
#pragma unroll
	for (int i = 0; i < EPT; i++) v[i] = sv[tid * EPT + i];
	for (int k = 2; k <= n; k <<= 1) {
		int j = k >> 1;
		if (j >= 64 * EPT) {
#pragma unroll
			for (int i = 0; i < EPT; i++) sv[tid * EPT + i] = v[i];
			__syncthreads();
			for (; j >= 64 * EPT; j >>= 1) {
				for (int t = tid; t < (n >> 1); t += 256) prune_ce(sv, t, j, k);
				__syncthreads();
			}
#pragma unroll
			for (int i = 0; i < EPT; i++) v[i] = sv[tid * EPT + i];
		}
		for (; j >= EPT; j >>= 1) {
			const int lx = j / EPT;
			const bool lower = (tid & lx) == 0;
#pragma unroll
			for (int i = 0; i < EPT; i++) {
				const bool desc = ((tid * EPT + i) & k) == 0;
				const W o = __shfl_xor(v[i], lx, 64);
				const W hi = v[i] > o ? v[i] : o, lo = v[i] > o ? o : v[i];
				v[i] = (lower == desc) ? hi : lo;
			}
		}
#pragma unroll
		for (int jj = EPT / 2; jj > 0; jj >>= 1) {
			if (jj <= (k >> 1)) {
#pragma unroll
				for (int i = 0; i < EPT; i++) {
					if ((i & jj) == 0) {
						const bool desc = ((tid * EPT + i) & k) == 0;
						const W x = v[i], y = v[i | jj];
						const W hi = x > y ? x : y, lo = x > y ? y : x;
						v[i]      = desc ? hi : lo;
						v[i | jj] = desc ? lo : hi;
					}
				}
			}
		}
	}
#pragma unroll
	for (int i = 0; i < EPT; i++) sv[tid * EPT + i] = v[i];
	__syncthreads();
}

template <class W>
__device__ __forceinline__ void prune_sort(W* sv, int n, int tid)
{
	switch (n) {
	case 256:  prune_sort_regs<1>(sv, tid); break;
	case 512:  prune_sort_regs<2>(sv, tid); break;
	case 1024: prune_sort_regs<4>(sv, tid); break;
	case 2048: prune_sort_regs<8>(sv, tid); break;
	case 4096: prune_sort_regs<16>(sv, tid); break;
	default:   prune_bitonic(sv, n, tid);
	}
}

// The sort words of k_prune_merge are 32 bits wide: the top bits of a (positive) weight — exponent and leading mantissa
// bits, as many as the slot leaves: 22 for up to 1024 emitted components, relative difference below 1e-3 inside a key —
// then the slot. Half the shuffles and compares of the 64-bit words above; the runs of equal keys are a little longer
// (they are ordered by the full weights afterwards, as there). 0 sorts last (padding); no real word is 0.
__device__ __forceinline__ unsigned int prune_pack32(double w, int slot, int sbits)
{
	const int kbn = 32 - sbits;
	unsigned int kb = (unsigned int) (((unsigned long long) __double_as_longlong(w) << 1) >> (64 - kbn));
	const unsigned int top = (1u << kbn) - 2u;
	kb = (kb > top ? top : kb) + 1u;
	return (kb << sbits) | (unsigned int) slot;
}
// the 32 bits of the weight behind those of the key
__device__ __forceinline__ unsigned int prune_next32(double w, int sbits)
{
	return (unsigned int) ((((unsigned long long) __double_as_longlong(w) << 1) << (32 - sbits)) >> 32);
}

// ---- what the phases share ---------------------------------------------------------------------------------------------------------
// One particle's run through the body: what every phase reads.
struct PruneRun {
	int p, tid, lane, wv;
	int ne;              // emitted entries
	int cut;             // rows kept (weightcut: every emitted weight is already >= MinWeight)
	size_t eb;           // the particle's place in the emitted list
	double* srec;        // [cutcap][PRUNE_ROW] the kept records in sorted order: component record (w, mean, covariance), canonical index, spare
	double merge_thr2;   // (a copy: a lambda that captured `prm` by reference would pin the argument block to memory)
#ifdef PHD_STAMPS
	long long* stamp_;
#endif
};
#ifdef PHD_STAMPS
#define PRUNE_STAMPS_OF(c) long long* const stamp_ = (c).stamp_
#else
#define PRUNE_STAMPS_OF(c)
#endif

// the mean of slab row r: the 32 bytes at its head, one sector
__device__ __forceinline__ void prune_slab_mean(const double* srec, int r, double& x0, double& x1, double& x2)
{
	const double2* row = (const double2*) (srec + (size_t) r * PRUNE_ROW);
	const double2 u0 = row[0], u1 = row[1];
	x0 = u0.y; x1 = u1.x; x2 = u1.y;
}
// the mean and the inverse covariance of slab row i: what the exact test needs of the row it is made for
__device__ __forceinline__ void prune_row_inverse(const double* srec, int i, double& m0, double& m1, double& m2, double* Pi)
{
	double P[6], mm[3], wi, det;
	load_comp(srec + (size_t) i * PRUNE_ROW, wi, mm, P);
	inv_sym3(P, Pi, det);
	m0 = mm[0]; m1 = mm[1]; m2 = mm[2];
}
// The exact closeness test of row i (inverse covariance Pi, Euclidean bound `bound`) and a row at distance d: the bound first, then
// Gaussian.SquareMahalanobis(b.Mean) < threshold^2
__device__ __forceinline__ bool prune_close(const double* Pi, double d0, double d1, double d2, double bound, double merge_thr2)
{
	const double sq = d0 * d0 + d1 * d1 + d2 * d2;
	return sq <= bound && quad_sym(Pi, d0, d1, d2) < merge_thr2;
}
// The float32 distance below which a candidate takes the exact test: float32 copies of the means relative to the box corner are within
// ferr of the true distance
__device__ __forceinline__ float prune_thr32(double bound, double ferr)
{
	const double rr = sqrt(bound) + ferr;
	return (float) (rr * rr * (1.0 + 1e-5));
}
// one more close row v of a row: the 7 smallest row numbers are kept, ascending (insertion through a fixed network; e is statically indexed only)
__device__ __forceinline__ void prune_keep7(unsigned int (&e)[PRUNE_NBR], int& cnt, unsigned int v)
{
#pragma unroll
	for (int q = 0; q < PRUNE_NBR; q++) {
		unsigned int lo_ = min(e[q], v), hi_ = max(e[q], v);
		e[q] = lo_; v = hi_;
	}
	cnt++;
}
// A row's two `nbr` words: the count of its close later rows (16 bits), then the first 7 of them, 16 bits each
__device__ __forceinline__ void prune_nbr_store(unsigned long long* nbr, int i, int cnt, const unsigned int (&e)[PRUNE_NBR])
{
	unsigned long long lo = (unsigned long long) min(cnt, 0xffff), hi = 0;
#pragma unroll
	for (int q = 0; q < PRUNE_NBR; q++) {
		if (q < cnt) {
			if (q < 3) lo |= (unsigned long long) e[q] << (16 * (q + 1));
			else hi |= (unsigned long long) e[q] << (16 * (q - 3));
		}
	}
	nbr[2 * i]     = lo;
	nbr[2 * i + 1] = hi;
}
__device__ __forceinline__ int prune_nbr_at(unsigned long long lo, unsigned long long hi, int c)
{
	return (int) (((c < 3) ? (lo >> (16 * (c + 1))) : (hi >> (16 * (c - 3)))) & 0xffff);
}
// The absorbed flags: bit s of lane l's (or absb[l]'s) word <-> row s * 64 + l. 64 slots of 64 rows: every cut phd_create admits (the
// LDS bounds MaxQuantity to some 3400 rows, prune_lds)
__device__ __forceinline__ bool prune_absorbed(unsigned long long word, int slot) { return (word >> slot) & 1ull; }

// Hash of a grid cell. The low three bits are the parities of the cell coordinates, so the 2 x 2 x 2 cells a
// ball meets always fall into 8 different buckets (no bucket is walked twice); the rest mixes the halved
// coordinates. Cells outside the box hash like any other: whatever they collide with fails the distance test.
constexpr unsigned int PRUNE_HA = 73856093u, PRUNE_HB = 19349663u, PRUNE_HC = 83492791u;
__device__ __forceinline__ int prune_bucket(int cx, int cy, int cz)
{
	const unsigned int h = (unsigned int) (cx >> 1) * PRUNE_HA ^ (unsigned int) (cy >> 1) * PRUNE_HB ^ (unsigned int) (cz >> 1) * PRUNE_HC;
	return (int) (((h & (PRUNE_NB / 8 - 1)) << 3) | (cx & 1) | ((cy & 1) << 1) | ((cz & 1) << 2));
}
// the 8 bucket ranges of a row (its float32 coordinates relative to the box) as start | length << 16; returns the total
__device__ __forceinline__ int prune_ranges(const unsigned short* cstart, double icell, const float4& me, unsigned int* qb)
{
	const int bx = (int) floor((double) me.x * icell - 0.5), by = (int) floor((double) me.y * icell - 0.5),
	          bz = (int) floor((double) me.z * icell - 0.5);
	const unsigned int xa0 = (unsigned int) (bx >> 1) * PRUNE_HA, xa1 = (unsigned int) ((bx + 1) >> 1) * PRUNE_HA;
	const unsigned int yb0 = (unsigned int) (by >> 1) * PRUNE_HB, yb1 = (unsigned int) ((by + 1) >> 1) * PRUNE_HB;
	const unsigned int zc0 = (unsigned int) (bz >> 1) * PRUNE_HC, zc1 = (unsigned int) ((bz + 1) >> 1) * PRUNE_HC;
	const int par0 = (bx & 1) | ((by & 1) << 1) | ((bz & 1) << 2);
	int n = 0;
#pragma unroll
	for (int c = 0; c < 8; c++) {
		const unsigned int h = ((c & 1) ? xa1 : xa0) ^ ((c & 2) ? yb1 : yb0) ^ ((c & 4) ? zc1 : zc0);
		const int bk = (int) ((h & (PRUNE_NB / 8 - 1)) << 3) | (par0 ^ c);   // neighbours flip the parity bits
		const int s0 = cstart[bk], n0 = cstart[bk + 1] - s0;
		qb[c] = (unsigned int) s0 | ((unsigned int) n0 << 16);
		n += n0;
	}
	return n;
}
// Every row of this thread with its mean relative to the box corner mn: rows tid + 256 q, q < 4, from the registers the gather left
// them in; beyond 1024 kept entries, back from the slab row
template <class F>
__device__ __forceinline__ void prune_each_row(const PruneRun& c, const double (&kmean)[4][3], double mn0, double mn1, double mn2, F f)
{
#pragma unroll
	for (int q = 0; q < 4; q++) {
		if (c.tid + 256 * q < c.cut) f(c.tid + 256 * q, kmean[q][0] - mn0, kmean[q][1] - mn1, kmean[q][2] - mn2);
	}
	for (int r = c.tid + 1024; r < c.cut; r += 256) {
		double x0, x1, x2;
		prune_slab_mean(c.srec, r, x0, x1, x2);
		f(r, x0 - mn0, x1 - mn1, x2 - mn2);
	}
}

// ---- A. order by (weight desc, canonical index asc) --------------------------------------------------------------------------------
// What A hands to the gather: row r of the sorted order is
//   listed: the emitted slot order[r] & smask (the sort words);
//   ranked: the place order[r] in the pool's kw | ks | ki, where the entry's key (= its weight), its slot and its canonical index are —
//           the gather then needs no trip to memory before the record's own.
struct PruneOrder {
	const unsigned int* order;
	unsigned int smask;
	bool ranked;
};
__device__ __forceinline__ PruneOrder prune_order(const StepBufs& a, const PruneLds& lay, const PrunePool& L, const PruneRun& c, double minw)
{
	PRUNE_STAMPS_OF(c);
	const int tid = c.tid, lane = c.lane, wv = c.wv, ne = c.ne, cut = c.cut, NS = lay.NS;
	const size_t eb = c.eb;
	unsigned int* const sw = L.sw;
	unsigned int* const w2 = L.w2;
	int sbits = 1;
	while ((1 << sbits) < ne) sbits++;                    // bits of a slot number
	const unsigned int smask = (1u << sbits) - 1u;
	int n = 256;                                      // (at least the width of the register sort: small maps, too, skip the barrier-per-stage version)
	while (n < ne && n < NS) n <<= 1;                 // width of the first pass
	int taken = 0;                                    // emitted entries consumed so far
	bool first = true, prefilled = false;
	PruneOrder o{sw, smask, false};
	// Only the `cut` heaviest entries are kept. A histogram over the weights' leading bits (exponent and five mantissa
	// bits, counted from MinWeight up: every emitted weight is at least that) finds the bin the cut-th heaviest entry lies
	// in; whole bins are taken, so nothing changes in the order of what is kept.
	//   * ranked: the entries from that bin up are scattered to their bins' places (a counting sort: the bins' starts are
	//     the suffix sums of the histogram) and every entry counts, among the few entries of its own bin, those that
	//     go before it — by the full weight, then the canonical index: the reference's sort made stable, with no sorting
	//     network, no runs of equal keys to order afterwards;
	//   * when that does not fit (more entries than the LDS arrays hold, or a bin crowded with hundreds of equal weights):
	//     the entries from the threshold bin up are sorted in one pass of the smallest width (more than 1024 emitted), or
	//     everything goes through the passes below.
	const int capN = lay.capN;
	if (ne > 256 && cut > 0) {
		int* const hist = L.hist;   // counts, then starts, then ends of the bins
		constexpr int BINS = PruneLds::BINS;
		static_assert(BINS == 1024, "the histogram's scan gives 16 bins to each of 64 lanes, weight_bin_of_bits clamps to 1023");
		int& s_T = hist[BINS];
		int& s_cnt = hist[BINS + 1];
		int& s_fill = hist[BINS + 2];
		int& s_maxb = hist[BINS + 3];
		unsigned int* const out = L.out;
		const unsigned int base = weight_bin_base(minw);
		auto bin_of_bits = [&](unsigned long long bits) { return weight_bin_of_bits(bits, base); };   // (phd_device.h: the emit body's cut floor counts into the same bins)
		auto bin_of = [&](double w) { return bin_of_bits((unsigned long long) __double_as_longlong(w)); };
		for (int t = tid; t < BINS + 4; t += 256) hist[t] = 0;
		__syncthreads();
		// (up to 2048 emitted entries a thread keeps its weights for the scatter below: one trip to memory instead of two)
		constexpr int WK = 8;
		const bool keepw = ne <= 256 * WK;
		// (their canonical indices — which decide between equal weights: components never detected since birth, dozens of
		// them — are kept beside the slots, and fetched HERE, with the weights, in one trip: read one by one inside the
		// scatter below they were a dependent trip to memory per entry, five in a row per thread)
		double wk[WK];
		int    ik[WK];
#pragma unroll
		for (int q = 0; q < WK; q++) {
			const int e = tid + 256 * q;
			wk[q] = (keepw && e < ne) ? a.emit_w[eb + e] : 0.0;
			ik[q] = (keepw && e < ne) ? a.emit_idx[eb + e] : 0;
		}
		if (keepw) {
#pragma unroll
			for (int q = 0; q < WK; q++) {
				if (tid + 256 * q < ne) atomicAdd(&hist[bin_of(wk[q])], 1);
			}
		}
		else {
			for (int e0 = tid; e0 < ne; e0 += 256 * WK) {
				double wr[WK];
#pragma unroll
				for (int q = 0; q < WK; q++) wr[q] = (e0 + 256 * q < ne) ? a.emit_w[eb + e0 + 256 * q] : 0.0;
#pragma unroll
				for (int q = 0; q < WK; q++) {
					if (e0 + 256 * q < ne) atomicAdd(&hist[bin_of(wr[q])], 1);
				}
			}
		}
		__syncthreads();
		if (wv == 0) {
			// from the top bin down (lane l: bins BINS - 1 - 16 l .. BINS - 16 - 16 l): every bin's count gives way to its start, the
			// number of entries in the bins above it; the first bin at which `cut` entries are reached is the threshold
			int cq[16], mine = 0;
#pragma unroll
			for (int q = 0; q < 16; q++) { cq[q] = hist[BINS - 1 - (16 * lane + q)]; mine += cq[q]; }
			int run = wave_incl_scan(mine) - mine, mxb = 0;
#pragma unroll
			for (int q = 0; q < 16; q++) {
				const int bq = BINS - 1 - (16 * lane + q);
				hist[bq] = run;
				if (run < cut) {
					mxb = max(mxb, cq[q]);
					if (cut <= run + cq[q]) { s_T = bq; s_cnt = run + cq[q]; }
				}
				run += cq[q];
			}
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) mxb = max(mxb, __shfl_xor(mxb, o, 64));
			if (lane == 0) s_maxb = mxb;
		}
		__syncthreads();
		const int T = s_T, cnt = s_cnt;
		if (cnt <= capN && s_maxb <= 512) {
			unsigned long long* const kw = L.kw;
			unsigned int* const ks = L.ks;
			unsigned int* const ki = L.ki;
			auto place = [&](double w, int e, int idx) {
				const int bq = bin_of(w);
				if (bq >= T) {
					const int pos = atomicAdd(&hist[bq], 1);   // (the start becomes the end)
					kw[pos] = prune_key(w);
					ks[pos] = (unsigned int) e;
					ki[pos] = (unsigned int) idx;
				}
			};
			if (keepw) {
#pragma unroll
				for (int q = 0; q < WK; q++) {
					if (tid + 256 * q < ne) place(wk[q], tid + 256 * q, ik[q]);
				}
			}
			else {
				// more than 2048 emitted entries: the same in rounds of WK entries per thread, a round's loads issued together
				for (int e0 = tid; e0 < ne; e0 += 256 * WK) {
#pragma unroll
					for (int q = 0; q < WK; q++) {
						const int e = e0 + 256 * q;
						wk[q] = (e < ne) ? a.emit_w[eb + e] : 0.0;
						ik[q] = (e < ne) ? a.emit_idx[eb + e] : 0;
					}
#pragma unroll
					for (int q = 0; q < WK; q++) {
						if (e0 + 256 * q < ne) place(wk[q], e0 + 256 * q, ik[q]);
					}
				}
			}
			__syncthreads();
			PHD_STAMP(6);
			for (int pos = tid; pos < cnt; pos += 256) {
				const unsigned long long key = kw[pos];
				const int bq = bin_of_bits(key);
				const int f0 = (bq == BINS - 1) ? 0 : hist[bq + 1], f1 = hist[bq];
				int rank = 0, ties = 0;
				for (int f = f0; f < f1; f += 4) {   // four bin-mates per trip, their keys fetched together
					unsigned long long kf[4];
#pragma unroll
					for (int q = 0; q < 4; q++) kf[q] = kw[min(f + q, f1 - 1)];
#pragma unroll
					for (int q = 0; q < 4; q++) {
						const bool in = f + q < f1;
						rank += (in && kf[q] > key) ? 1 : 0;
						ties += (in && kf[q] == key) ? 1 : 0;
					}
				}
				if (ties > 1) {   // others with this very weight: the canonical index decides
					const int myidx = (int) ki[pos];
					for (int f = f0; f < f1; f++) {
						if (f != pos && kw[f] == key) {
							const int fidx = (int) ki[f];
							if (fidx < myidx) rank++;
						}
					}
				}
				out[f0 + rank] = (unsigned int) pos;
			}
			__syncthreads();
			PHD_STAMP(11);
			o.order = out;
			o.ranked = true;
		}
		else if (ne > 1024 && cnt <= NS) {   // (else: a crowd of equal weights at the cut — the passes below take everything)
			n = 256;
			while (n < cnt) n <<= 1;
			for (int e = tid; e < ne; e += 256) {
				const double w = a.emit_w[eb + e];
				if (e < NS) w2[e] = prune_next32(w, sbits);
				if (bin_of(w) >= T) sw[atomicAdd(&s_fill, 1)] = prune_pack32(w, e, sbits);
			}
			for (int t = cnt + tid; t < n; t += 256) sw[t] = 0u;
			taken = ne;
			prefilled = true;
		}
	}
	while (!o.ranked && (first || taken < ne)) {
		// first pass: fill [0, n); later passes (n == NS): refill the worse half [n/2, n)
		const int from = first ? 0 : (n >> 1);
		for (int t = from + tid; t < n && !prefilled; t += 256) {
			int e = taken + (t - from);
			unsigned int word = 0u;
			if (e < ne) {
				const double w = a.emit_w[eb + e];
				word = prune_pack32(w, e, sbits);
				if (e < NS) w2[e] = prune_next32(w, sbits);
			}
			sw[t] = word;
		}
		if (!prefilled) taken += n - from;
		first = false;
		__syncthreads();
		PHD_STAMP(6);    // (the last pass: fill | sort | runs)
		prune_sort(sw, n, tid);
		PHD_STAMP(11);
		// runs that agree in the key bits: order by (weight desc, canonical index asc); the thread at the
		// head of a run sorts it (runs are disjoint)
		for (int r = tid; r + 1 < n; r += 256) {
			const unsigned int kb = sw[r] >> sbits;
			if (sw[r + 1] == 0u || (sw[r + 1] >> sbits) != kb || (r > 0 && (sw[r - 1] >> sbits) == kb)) continue;
			int e = r + 2;
			while (e < n && sw[e] != 0u && (sw[e] >> sbits) == kb) e++;
			// (the 32 weight bits behind the key decide nearly every pair: they are in LDS; the full weights and the
			// canonical indices, a dependent HBM access each, only behind a tie in all 54 bits)
			auto next32 = [&](int sl) { return sl < NS ? w2[sl] : prune_next32(a.emit_w[eb + sl], sbits); };
			for (int x = r + 1; x < e; x++) {   // insertion sort of the run
				const unsigned int vx = sw[x];
				const int sx = (int) (vx & smask);
				const unsigned int nx = next32(sx);
				int y = x - 1;
				while (y >= r) {
					const int sy = (int) (sw[y] & smask);
					const unsigned int ny = next32(sy);
					bool stays = ny > nx;   // sy stays before sx
					if (ny == nx) {
						const double wy = a.emit_w[eb + sy], wx = a.emit_w[eb + sx];
						stays = wy > wx || (wy == wx && a.emit_idx[eb + sy] < a.emit_idx[eb + sx]);
					}
					if (stays) break;
					sw[y + 1] = sw[y];
					y--;
				}
				sw[y + 1] = vx;
			}
		}
		__syncthreads();
	}
	return o;
}

// ---- S. the kept records, gathered once into sorted order (the slab's 96-byte rows in HBM); the Euclidean bounds go to LDS ---------
// A pair can only be close when |m_i - m_k|^2 <= T^2 trace(P_i) (d^T P_i^-1 d >= |d|^2 / lambda_max(P_i) >=
// |d|^2 / trace(P_i) for a positive definite P_i).
// Leaves: the slab, rad2, the means of this thread's first four rows (kmean: all rows, up to 1024 kept entries — they stay in registers
// for the grid), and per wave in `bred` the box of the means and the largest radius, all seven as maxima.
__device__ __forceinline__ void prune_gather(const DevParams& prm, const StepBufs& a, const PrunePool& L, const PruneRun& c, const PruneOrder& o,
                                             double (&kmean)[4][3])
{
	const int p = c.p, tid = c.tid, lane = c.lane, wv = c.wv, cut = c.cut;
	const size_t eb = c.eb;
	double* const srec = c.srec;
	float* const rad2 = L.rad2;
	const double merge_thr2 = c.merge_thr2;
	const unsigned int* const order = o.order;
	double lo0 = INFINITY, lo1 = INFINITY, lo2 = INFINITY, hi0 = -INFINITY, hi1 = -INFINITY, hi2 = -INFINITY, rmx = 0;
	const MixView vpre = bank_view(a, SEL_IN);
	const int nprior = vpre.count[p], npredicted = nprior + a.born_count[p];
	const double* prior = vpre.rec + in_base(a, p) * MIX_REC;
	// Row r of the sorted order: where it comes from. A misdetection copy (canonical index below the size of the predicted
	// mixture, PHDNavigator.cs:837-840) IS the predicted component with another weight: its record is read where it is, in the
	// prior bank (a birth's is made up); a detection update's record is the one k_emit_finish wrote. Either is one 80-byte
	// record. First the rows' descriptions (LDS on the ranked path, the emitted list otherwise), then their records: the
	// two trips of a thread's rows overlap.
	double birthP[6];
#pragma unroll
	for (int t = 0; t < 6; t++) birthP[t] = prm.birthP[t];   // (a local copy, as merge_thr2: the lambdas below must not capture `prm`)
	// The gather is written WITHOUT control flow between a thread's loads: behind a divergent branch the compiler waits for
	// every outstanding memory operation (s_waitcnt vmcnt(0) at the join — it cannot count them across the branch), which made
	// a thread's rows one full trip to memory each, one after the other. Rows beyond the cut are clamped to the last kept row
	// (their loads hit lines the wave reads anyway, their stores are predicated off); a birth's copy reads its (unwritten)
	// emit record like an update and is patched afterwards (rare: the one branch, behind all loads).
	struct RowSrc { const double* rec; double w; int cidx; };
	auto resolve_ranked = [&](int r) {
		RowSrc s;
		const unsigned int pos = order[r];
		const int slt = (int) L.ks[pos];
		s.w = __longlong_as_double((long long) (L.kw[pos] & 0x7fffffffffffffffull));   // prune_key of a positive weight, undone
		s.cidx = (int) L.ki[pos];
		s.rec = (s.cidx < nprior) ? prior + (size_t) s.cidx * MIX_REC : a.emit_rec + (eb + slt) * MIX_REC;
		return s;
	};
	auto resolve_listed = [&](int slt, double w, int cidx) {
		RowSrc s;
		s.w = w; s.cidx = cidx;
		s.rec = (cidx < nprior) ? prior + (size_t) cidx * MIX_REC : a.emit_rec + (eb + slt) * MIX_REC;
		return s;
	};
	struct RowRec { double m0, m1, m2, P0, P1, P2, P3, P4, P5; };
	auto fetch = [&](const RowSrc& s) {   // (five 16-byte loads; the weight in front of the mean is the entry's own, s.w)
		const double2* q = (const double2*) s.rec;
		const double2 a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4];
		return RowRec{a0.y, a1.x, a1.y, a2.x, a2.y, a3.x, a3.y, a4.x, a4.y};
	};
	// the copy of a birth (canonical index in [nprior, npredicted)): mean from the sweep, BirthCovariance — selects, no branch
	auto patch_birth = [&](const RowSrc& s, RowRec v) {
		const bool birth = s.cidx >= nprior && s.cidx < npredicted;
		const double* bm = a.born_mean + ((size_t) p * a.Mcap + (birth ? s.cidx - nprior : 0)) * 3;
		const double b0 = bm[0], b1 = bm[1], b2 = bm[2];
		v.m0 = birth ? b0 : v.m0; v.m1 = birth ? b1 : v.m1; v.m2 = birth ? b2 : v.m2;
		v.P0 = birth ? birthP[0] : v.P0; v.P1 = birth ? birthP[1] : v.P1; v.P2 = birth ? birthP[2] : v.P2;
		v.P3 = birth ? birthP[3] : v.P3; v.P4 = birth ? birthP[4] : v.P4; v.P5 = birth ? birthP[5] : v.P5;
		return v;
	};
	// ... its record into the slab; its bound into LDS; the box and the largest radius
	auto stage = [&](int r, const RowSrc& s, const RowRec& v) {
		double2* row = (double2*) (srec + (size_t) r * PRUNE_ROW);
		row[0] = make_double2(s.w, v.m0); row[1] = make_double2(v.m1, v.m2);
		row[2] = make_double2(v.P0, v.P1); row[3] = make_double2(v.P2, v.P3); row[4] = make_double2(v.P4, v.P5);
		row[5] = make_double2((double) s.cidx, 0.0);
		const double det = v.P0 * (v.P3 * v.P5 - v.P4 * v.P4) - v.P1 * (v.P1 * v.P5 - v.P4 * v.P2) + v.P2 * (v.P1 * v.P4 - v.P3 * v.P2);
		const bool pd = v.P0 > 0 && (v.P0 * v.P3 - v.P1 * v.P1) > 0 && det > 0;   // Sylvester
		const double rad = pd ? sqrt(merge_thr2 * (v.P0 + v.P3 + v.P5)) : INFINITY;
		{
			const double b2 = rad * rad * (1.0 + 1e-6);
			float bf = (float) b2;
			if ((double) bf < b2) bf = __int_as_float(__float_as_int(bf) + 1);   // (positive, finite: the next float32 up; +inf converts to +inf)
			rad2[r] = bf;
		}
		rmx = pd ? fmax(rmx, rad) : rmx;
		lo0 = fmin(lo0, v.m0); lo1 = fmin(lo1, v.m1); lo2 = fmin(lo2, v.m2);
		hi0 = fmax(hi0, v.m0); hi1 = fmax(hi1, v.m1); hi2 = fmax(hi2, v.m2);
	};
	// Two rows of this thread per batch (ra, ra + 256): both descriptions, then both records, then the stores — vector memory
	// operations retire in issue order (vmcnt counts loads and stores together), so no load is issued behind a store of its
	// own batch. (Four rows per batch: the kernel spilled 192 bytes per lane at its 128 registers.)
#pragma unroll
	for (int q = 0; q < 4; q++) { kmean[q][0] = 0; kmean[q][1] = 0; kmean[q][2] = 0; }
	const bool anybirth = npredicted > nprior;
	auto gather2 = [&](int ra, double* ka, double* kb) {
		const int rb = ra + 256;
		const int ca = min(ra, cut - 1), cb = min(rb, cut - 1);
		RowSrc oa, ob;
		if (o.ranked) {   // (workgroup-uniform)
			oa = resolve_ranked(ca); ob = resolve_ranked(cb);
		}
		else {
			const int sa = (int) (order[ca] & o.smask), sb = (int) (order[cb] & o.smask);
			const double wa = a.emit_w[eb + sa], wb = a.emit_w[eb + sb];
			const int ia = a.emit_idx[eb + sa], ib = a.emit_idx[eb + sb];
			oa = resolve_listed(sa, wa, ia); ob = resolve_listed(sb, wb, ib);
		}
		RowRec va = fetch(oa), vb = fetch(ob);
		if (anybirth) { va = patch_birth(oa, va); vb = patch_birth(ob, vb); }   // (workgroup-uniform)
		if (ra < cut) { stage(ra, oa, va); if (ka) { ka[0] = va.m0; ka[1] = va.m1; ka[2] = va.m2; } }
		if (rb < cut) { stage(rb, ob, vb); if (kb) { kb[0] = vb.m0; kb[1] = vb.m1; kb[2] = vb.m2; } }
	};
	if (cut > 0) {
		gather2(tid, kmean[0], kmean[1]);
		if (cut > 512) gather2(tid + 512, kmean[2], kmean[3]);
		for (int ra = tid + 1024; ra < cut; ra += 512) gather2(ra, nullptr, nullptr);
	}
	double red7[7] = {-lo0, -lo1, -lo2, hi0, hi1, hi2, rmx};   // all as maxima
#pragma unroll
	for (int q = 0; q < 7; q++) {
#pragma unroll
		for (int s = 32; s > 0; s >>= 1) red7[q] = fmax(red7[q], __shfl_xor(red7[q], s, 64));
	}
	if (lane == 0) {
#pragma unroll
		for (int q = 0; q < 7; q++) L.bred[wv * 7 + q] = red7[q];
	}
}

// ---- B. all closeness tests close_i(k), k > i ----------------------------------------------------------------------------------------
// The rows are binned in a uniform grid of cell size 2 * (largest radius): the ball of a row then meets at most 2 x 2 x 2 cells, whose
// members are the only candidates. Rows whose P_i is not positive definite, or whose radius exceeds the cell bound, test every later row.
struct PruneGrid {
	double icell, rcap;   // 1 / cell size; the largest radius whose ball stays inside 2 x 2 x 2 cells
	double ferr;          // float32 copies of the means relative to the box corner are off by at most 2^-24 ext per coordinate, so a float32 distance is within ferr of the true one
	int hstart;           // the rows at the positions from hstart on in `ord` are left to the wave walk
};
// The grid (a counting sort of the rows by bucket into `cand`) and the order in which the pair search takes the rows (`ord`)
__device__ __forceinline__ PruneGrid prune_grid(const PrunePool& L, const PruneRun& c, const double (&kmean)[4][3])
{
	PRUNE_STAMPS_OF(c);
	const int tid = c.tid, lane = c.lane, wv = c.wv, cut = c.cut;
	float* const rad2 = L.rad2;
	float4* const cand = L.cand;
	int* const owner = L.owner;
	unsigned int* const cw = L.cw;
	unsigned short* const ord = L.ord;
	unsigned short* const rowpos = L.rowpos;
	int* const scan = L.scan;
	double red7[7];
#pragma unroll
	for (int q = 0; q < 7; q++) red7[q] = fmax(fmax(L.bred[q], L.bred[7 + q]), fmax(L.bred[14 + q], L.bred[21 + q]));
	const double mn0 = -red7[0], mn1 = -red7[1], mn2 = -red7[2];
	const double ext = fmax(red7[3] - mn0, fmax(red7[4] - mn1, red7[5] - mn2));
	double cell = fmax(2.02 * red7[6], ext / 60.0);   // <= 61 cells per axis
	if (!(cell > 0)) cell = 1.0;
	const double icell = 1.0 / cell, rcap = 0.5 * cell / 1.005;
	const double ferr = 4e-7 * ext;
	for (int t = tid; t < PruneLds::CW; t += 256) cw[t] = 0;
	__syncthreads();
	// counting sort of the rows by bucket (16-bit counters: cut <= 65535)
	prune_each_row(c, kmean, mn0, mn1, mn2, [&](int r, double s0, double s1, double s2) {
		const int b = prune_bucket((int) (s0 * icell), (int) (s1 * icell), (int) (s2 * icell));
		owner[r] = b;
		atomicAdd(&cw[b >> 1], 1u << (16 * (b & 1)));
	});
	__syncthreads();
	{   // inclusive prefix over the bucket counts: cstart[b] = end of bucket b; the fill below counts it down to its start
		constexpr int WT = PRUNE_NB / 2 / 256;   // words per thread
		unsigned int wd[WT];
		int tot = 0;
#pragma unroll
		for (int u = 0; u < WT; u++) { wd[u] = cw[WT * tid + u]; tot += (int) (wd[u] & 0xffff) + (int) (wd[u] >> 16); }
		const int incl = wave_incl_scan(tot);
		if (lane == 63) scan[wv] = incl;
		__syncthreads();
		int run = incl - tot;
		for (int q = 0; q < wv; q++) run += scan[q];
#pragma unroll
		for (int u = 0; u < WT; u++) {
			const int e0 = run + (int) (wd[u] & 0xffff), e1 = e0 + (int) (wd[u] >> 16);
			cw[WT * tid + u] = (unsigned int) e0 | ((unsigned int) e1 << 16);
			run = e1;
		}
		if (tid == 0) cw[PRUNE_NB / 2] = (unsigned int) cut;   // cstart[NB]: the end of the last bucket
	}
	__syncthreads();
	prune_each_row(c, kmean, mn0, mn1, mn2, [&](int r, double s0, double s1, double s2) {
		const int b = owner[r], sh = 16 * (b & 1);
		const int pos = (int) ((atomicSub(&cw[b >> 1], 1u << sh) >> sh) & 0xffff) - 1;
		cand[pos] = make_float4((float) s0, (float) s1, (float) s2, __int_as_float(r));
		rowpos[r] = (unsigned short) pos;
		owner[r] = -1;
	});
	__syncthreads();
	PHD_STAMP(7);

	// The rows are handed to the lanes in the order of their candidate counts (the rows of the 8 buckets their ball
	// meets; cells near the sensor hold an order of magnitude more rows than the rest): a wave then walks as long as
	// its rows need on average, not as long as the one unlucky row in it. Counting sort by min(count, 63); 63 also
	// stands for the rows that must test every later row.
	// (the row's own float32 coordinates, from its record in `cand`: 2^-24 of the extent away from the true ones, far
	// inside the margin rcap leaves between a ball and the 2 x 2 x 2 cells around it — no global load in this part)
	int* hist = scan;   // [64]
	if (tid < 64) hist[tid] = 0;
	__syncthreads();
	for (int i = tid; i < cut; i += 256) {
		int key = 63;
		if ((double) rad2[i] <= rcap * rcap) {
			unsigned int qb[8];
			key = min(prune_ranges(L.cstart, icell, cand[rowpos[i]], qb), 62);
		}
		owner[i] = key;
		atomicAdd(&hist[key], 1);
	}
	__syncthreads();
	if (tid < 64) {   // hist[key] = first position of the rows with that key, lightest first: thread t takes the positions
		// t, t + 256, ..., so the waves that get a last, partial round of the heaviest rows started with the lightest
		const int h = hist[tid];
		hist[tid] = wave_incl_scan(h) - h;
	}
	__syncthreads();
	for (int i = tid; i < cut; i += 256) {
		ord[atomicAdd(&hist[owner[i]], 1)] = (unsigned short) i;
		owner[i] = -1;
	}
	__syncthreads();
	PHD_STAMP(8);
	// hist[key] now ends key's rows: the rows with more than PRUNE_HEAVY candidates (and those on the full scan) sit
	// at the positions from hstart on. One lane would walk such a row for a hundred trips while its wave waits, so
	// they are left to the wave walk, where a wave spreads one row's candidates over its lanes.
	return PruneGrid{icell, rcap, ferr, hist[PRUNE_HEAVY]};
}

// ---- C. who survives: sequential in rank order, one wave, absorbed bits in registers -------------------------------------------------
__device__ __forceinline__ void prune_resolve(const PrunePool& L, const PruneRun& c)
{
	const int lane = c.lane, cut = c.cut;
	int* const owner = L.owner;
	auto readlane64 = [](unsigned long long v, int l) {   // (l wave-uniform)
		return ((unsigned long long) (unsigned int) __builtin_amdgcn_readlane((int) (v >> 32), l) << 32) | (unsigned int) __builtin_amdgcn_readlane((int) (unsigned int) v, l);
	};
	if (c.wv != 0) return;
	unsigned long long absorbed = 0;            // this lane's word of the absorbed flags (prune_absorbed)
	const int nslots = (cut + 63) >> 6;
	for (int base = 0; base < cut; base += 64) {
		const int s0 = base >> 6;
		// this lane holds the record of row base + lane
		unsigned long long vlo = 0, vhi = 0;
		if (base + lane < cut) { vlo = L.nbr[2 * (base + lane)]; vhi = L.nbr[2 * (base + lane) + 1]; }
		const int lolo = (int) (unsigned int) vlo, lohi = (int) (unsigned int) (vlo >> 32);
		const int hilo = (int) (unsigned int) vhi, hihi = (int) (unsigned int) (vhi >> 32);
		// only rows that have close later rows can change anything: walk those, in order
		unsigned long long todo = ballot64((lolo & 0xffff) != 0);
		while (todo) {
			const int l = __ffsll((long long) todo) - 1;
			todo &= todo - 1;
			const int i = base + l;
			if (prune_absorbed(readlane64(absorbed, l), s0)) continue;
			const unsigned int w0 = (unsigned int) __builtin_amdgcn_readlane(lolo, l);
			const int cnt = (int) (w0 & 0xffff);
			if (cnt <= PRUNE_NBR) {
				const unsigned long long lo = ((unsigned long long) (unsigned int) __builtin_amdgcn_readlane(lohi, l) << 32) | w0;
				const unsigned long long hi = ((unsigned long long) (unsigned int) __builtin_amdgcn_readlane(hihi, l) << 32) |
				                              (unsigned int) __builtin_amdgcn_readlane(hilo, l);
				for (int q = 0; q < cnt; q++) {
					const int k = prune_nbr_at(lo, hi, q);
					if (!prune_absorbed(readlane64(absorbed, k & 63), k >> 6)) {
						if (lane == (k & 63)) absorbed |= 1ull << (k >> 6);
						if (lane == 0) owner[k] = i;
					}
				}
			}
			else {
				// more close rows than the list holds: re-test row i against every later row, 64 at a time. No Euclidean bound here, the
				// quadratic form alone (the reference's own test): the bound only ever spares the form, it never decides
				double m0, m1, m2, Pi[6];
				prune_row_inverse(c.srec, i, m0, m1, m2, Pi);
				for (int s = i >> 6; s < nslots; s++) {
					int k = s * 64 + lane;
					if (k > i && k < cut && !prune_absorbed(absorbed, s)) {
						double k0, k1, k2;
						prune_slab_mean(c.srec, k, k0, k1, k2);
						if (quad_sym(Pi, m0 - k0, m1 - k1, m2 - k2) < c.merge_thr2) {
							absorbed |= 1ull << s;
							owner[k] = i;
						}
					}
				}
			}
		}
	}
	L.absb[lane] = absorbed;
}

// PruneModel of the workgroup's particle: the five phases and the barriers between them
__device__ __forceinline__ void prune_merge_body(const DevParams& prm, const StepBufs& a, int cutcap, double* smem, long long tk0 = 0)
{
	const PruneLds lay = prune_lds(cutcap);
	const PrunePool L = prune_pool(smem, lay);
	// (the particle's number through an empty asm: in the fused launch the compiler otherwise computes this body's addresses at the
	// top of the kernel and carries them — spilled — across the emit body)
	int p_ = a.p0 + blockIdx.x;
	asm volatile("" : "+s"(p_));
	PHD_STAMP_DECL;
	PruneRun c;
	c.p = p_; c.tid = threadIdx.x; c.lane = c.tid & 63; c.wv = c.tid >> 6;
	const MixView vout = bank_view(a, SEL_OUT);
	c.ne = a.emit_count[c.p];
	c.eb = (size_t) c.p * a.ecap;
	c.merge_thr2 = prm.merge_thr2;
	c.cut = min(min(prm.maxq, c.ne), cutcap);
	c.srec = a.srec + (size_t) c.p * PRUNE_ROW * cutcap;
#ifdef PHD_STAMPS
	c.stamp_ = stamp_;
#endif
	// (for the blocks of this body)
	const int p = c.p, tid = c.tid, lane = c.lane, wv = c.wv, cut = c.cut;
	const double* const srec = c.srec;
	const float4* const cand = L.cand;
	const double merge_thr2 = c.merge_thr2;

	PHD_STAMP(0);
	const PruneOrder order = prune_order(a, lay, L, c, prm.minw);
	PHD_STAMP(1);
	double kmean[4][3];
	prune_gather(prm, a, L, c, order, kmean);
	__syncthreads();   // the sort words and the ranked arrays are dead from here on: the merge half takes their place
	PHD_STAMP(2);
	{
		const PruneGrid g = prune_grid(L, c, kmean);
		// ---- B, lane walk (a block of the body, not a function: see the file's head). The rows in front of hstart, one per lane: the
		// <= 8 buckets its ball meets are walked as one list of float32 records
		{
			const double rcap = g.rcap;
#ifdef PHD_STAMPS
			long long acc_setup = 0, acc_trips = 0, acc_drain = 0, tmark = clock64();
#endif
			for (int t = tid; t < g.hstart; t += 256) {
				const int i = L.ord[t];
				const float4 me = cand[L.rowpos[i]];
				const double bound = (double) L.rad2[i];
				int cnt = 0;
				unsigned int e[PRUNE_NBR];   // close rows found (statically indexed only)
#pragma unroll
				for (int q = 0; q < PRUNE_NBR; q++) e[q] = 0xffffu;
				// the row's own record (mean, P^-1) is needed by the exact test only, which few rows ever reach: loaded then
				bool have = false;
				double m0 = 0, m1 = 0, m2 = 0, Pi[6] = {0, 0, 0, 0, 0, 0};
				if (bound <= rcap * rcap) {
					const float fx = me.x, fy = me.y, fz = me.z;
					const float thr = prune_thr32(bound, g.ferr);
					unsigned long long pend0 = 0, pend1 = 0;   // up to 8 queued rows as 16-bit fields
					int npend = 0;
					// the queued rows' exact tests, four at a time: their means are fetched together (one trip to the slab for the
					// four, not one each, one after the other)
					auto drain = [&]() {
						if (npend > 0 && !have) {
							prune_row_inverse(srec, i, m0, m1, m2, Pi);
							have = true;
						}
						for (int b0 = 0; b0 < npend; b0 += 4) {
							int kk[4];
							double kx[4], ky[4], kz[4];
#pragma unroll
							for (int u = 0; u < 4; u++) {
								const int f = b0 + u;
								kk[u] = (f < npend) ? (int) (((f < 4) ? (pend0 >> (16 * f)) : (pend1 >> (16 * (f - 4)))) & 0xffff) : i;
								prune_slab_mean(srec, kk[u], kx[u], ky[u], kz[u]);   // (an idle slot reads the row's own mean: a line it has)
							}
#pragma unroll
							for (int u = 0; u < 4; u++) {
								if (b0 + u < npend && prune_close(Pi, m0 - kx[u], m1 - ky[u], m2 - kz[u], bound, merge_thr2)) prune_keep7(e, cnt, (unsigned int) kk[u]);
							}
						}
						npend = 0; pend0 = 0; pend1 = 0;
					};
					unsigned int qb[8];
					const int n = prune_ranges(L.cstart, g.icell, me, qb);
					// one candidate per trip, the 8 ranges one after the other. The exact test is rare per lane but not per
					// wave: a candidate that passes the float32 distance test is queued and tested later, so that the waves do
					// not run the FP64 path at every candidate
					// the non-empty ranges first, in their order (a stable compaction through static indices): the walk below then
					// moves to the next range with one predicated step instead of a loop over possibly empty ones
					unsigned int nz[8];
					{
						int before[8], run = 0;
#pragma unroll
						for (int u = 0; u < 8; u++) { before[u] = run; run += (qb[u] >> 16) ? 1 : 0; }
#pragma unroll
						for (int j = 0; j < 8; j++) {
							unsigned int v = 0;
#pragma unroll
							for (int u = j; u < 8; u++) v = ((qb[u] >> 16) && before[u] == j) ? qb[u] : v;
							nz[j] = v;
						}
					}
#ifdef PHD_STAMPS
					{ long long now = clock64(); acc_setup += now - tmark; tmark = now; }
#endif
					unsigned int cur = 0, left = 0;
					int cx = 0;
					// (four candidates per trip, their four LDS reads in flight together, was measured: the walk took 37 k cycles
					// against 19 k — the bookkeeping of four cursors with their divergent range changes costs more than the latency)
					for (int f = 0; f < n; f++) {
#ifdef PHD_STAMP_COUNTERS
						if (a.stamps && a.stamp_kernel == 2 && (int) (__ffsll((long long) ballot64(1)) - 1) == lane) atomicAdd(&a.stamps[(size_t) p * 16 + 15], 1.0);   // wave-level trips
#endif
						if (left == 0) {
							unsigned int q = nz[0];
#pragma unroll
							for (int u = 1; u < 8; u++) q = (cx == u) ? nz[u] : q;
							cx++;
							cur = q & 0xffff; left = q >> 16;
						}
						const float4 cd = cand[cur];
						cur++; left--;
						const int k = __float_as_int(cd.w);
						const float e0 = fx - cd.x, e1 = fy - cd.y, e2 = fz - cd.z;
						if (k > i && e0 * e0 + e1 * e1 + e2 * e2 <= thr) {
							if (npend < 4) pend0 |= (unsigned long long) k << (16 * npend);
							else           pend1 |= (unsigned long long) k << (16 * (npend - 4));
							npend++;
							if (npend > 7) drain();
						}
					}
#ifdef PHD_STAMPS
					{ long long now = clock64(); acc_trips += now - tmark; tmark = now; }
#endif
					drain();
#ifdef PHD_STAMPS
					{ long long now = clock64(); acc_drain += now - tmark; tmark = now; }
#endif
				}
				else {
					for (int k = i + 1; k < cut; k++) {
						if (!have) {
							prune_row_inverse(srec, i, m0, m1, m2, Pi);
							have = true;
						}
						double k0, k1, k2;
						prune_slab_mean(srec, k, k0, k1, k2);
						if (prune_close(Pi, m0 - k0, m1 - k1, m2 - k2, bound, merge_thr2)) prune_keep7(e, cnt, (unsigned int) k);
					}
				}
				prune_nbr_store(L.nbr, i, cnt, e);
#ifdef PHD_STAMP_COUNTERS   // (slow: contended atomics; counts only, never together with timing)
				if (a.stamps && a.stamp_kernel == 2) {
					atomicAdd(&a.stamps[(size_t) p * 16 + 14], (double) cnt);                               // close pairs
					unsigned int qd[8];
					atomicAdd(&a.stamps[(size_t) p * 16 + 13], (double) ((bound <= rcap * rcap) ? prune_ranges(L.cstart, g.icell, me, qd) : 0));     // candidates
				}
#endif
			}
#if defined(PHD_STAMPS) && !defined(PHD_STAMP_COUNTERS)   // (the counters' build uses the same slots for its counts)
			if (tid == 0 && a.stamps && a.stamp_kernel == 2) { a.stamps[(size_t) p * 16 + 12] = (double) acc_setup; a.stamps[(size_t) p * 16 + 13] = (double) acc_trips; a.stamps[(size_t) p * 16 + 14] = (double) acc_drain; }
#endif
		}
		PHD_STAMP(9);
		// ---- B, wave walk (a block, as the lane walk). The rows from hstart on, one crowded row per wave at a time, a candidate per lane
		{
			for (int h = g.hstart + wv; h < cut; h += 4) {   // (wave-uniform)
				const int i = L.ord[h];
				const float4 me = cand[L.rowpos[i]];
				const double bound = (double) L.rad2[i];
				int cnt = 0;
				unsigned int e[PRUNE_NBR];   // the same in every lane
#pragma unroll
				for (int q = 0; q < PRUNE_NBR; q++) e[q] = 0xffffu;
				bool have = false;
				double m0 = 0, m1 = 0, m2 = 0, Pi[6] = {0, 0, 0, 0, 0, 0};
				auto exact = [&](int k) {
					if (!have) {
						prune_row_inverse(srec, i, m0, m1, m2, Pi);
						have = true;
					}
					double k0, k1, k2;
					prune_slab_mean(srec, k, k0, k1, k2);
					return prune_close(Pi, m0 - k0, m1 - k1, m2 - k2, bound, merge_thr2);
				};
				auto collect = [&](bool close, int k) {   // the close rows found by the lanes, into the sorted list all lanes keep
					unsigned long long bal = ballot64(close);
					while (bal) {
						const int l = __ffsll((long long) bal) - 1;
						bal &= bal - 1;
						prune_keep7(e, cnt, (unsigned int) __shfl(k, l, 64));
					}
				};
				if (bound <= g.rcap * g.rcap) {
					const float thr = prune_thr32(bound, g.ferr);
					unsigned int qb[8];
					const int n = prune_ranges(L.cstart, g.icell, me, qb);
					for (int f0 = 0; f0 < n; f0 += 64) {
						const int f = f0 + lane;
						int rem = f;
						unsigned int cur = 0;
						bool found = false;
#pragma unroll
						for (int b = 0; b < 8; b++) {
							const int len = (int) (qb[b] >> 16);
							if (!found && rem < len) { cur = (qb[b] & 0xffff) + (unsigned int) rem; found = true; }
							else if (!found) rem -= len;
						}
						bool close = false;
						int k = 0;
						if (found) {
							const float4 cd = cand[cur];
							k = __float_as_int(cd.w);
							const float e0 = me.x - cd.x, e1 = me.y - cd.y, e2 = me.z - cd.z;
							if (k > i && e0 * e0 + e1 * e1 + e2 * e2 <= thr) close = exact(k);
						}
						collect(close, k);
					}
				}
				else {
					for (int k0 = i + 1; k0 < cut; k0 += 64) {
						const int k = k0 + lane;
						collect(k < cut && exact(k), k);
					}
				}
				if (lane == 0) prune_nbr_store(L.nbr, i, cnt, e);
			}
		}
	}
	PHD_STAMP(10);
	__syncthreads();
	PHD_STAMP(3);
	prune_resolve(L, c);
	__syncthreads();
	PHD_STAMP(4);
	// ---- D. output position of every survivor (exclusive scan of the survivor flags) and the merges ---------------------------------------
	// For the reweight (k_alpha_density): a survivor that absorbed nothing and is the misdetection copy of predicted
	// component c (canonical index c < np, PHDNavigator.cs:837-840) IS that component with another weight — Merge
	// (Gaussian.cs:329-346) of a single Gaussian changes its moments only by rounding, which is checked here —, so its
	// density at a landmark is the predicted component's times wcopy[c] / w_c. wcopy[c] = that weight (0: none such),
	// cover[pos] = 1 for the survivors accounted for this way.
	// (A block of the body, not a function: see the file's head.)
	const unsigned long long* const nbr = L.nbr;
	const int* const owner = L.owner;
	int* const scan = L.scan;
	const int npred = bank_of(a, SEL_IN).count[p] + a.born_count[p];
	double* wcopy = a.wcopy + (size_t) p * (a.cap + a.Mcap);
	for (int q = tid; q < npred; q += 256) wcopy[q] = 0.0;
	__syncthreads();
	// positions first, for all rows at once (one barrier): the survivors of every chunk of 256 rows and wave are counted into
	// scan[chunk][wave]; a survivor's position is the survivors of the chunks before its own, of the waves before its own in
	// the chunk, and of the lanes before its own in the wave
	const int nchunks = (cut + 255) >> 8;   // (at most 14: MaxQuantity is bounded by the LDS, phd_create)
	auto survives = [&](int i) { return i < cut && !prune_absorbed(L.absb[i & 63], i >> 6); };
	for (int q = 0; q < nchunks; q++) {
		const unsigned long long bal = ballot64(survives(q * 256 + tid));
		if (lane == 0) scan[q * 4 + wv] = __popcll(bal);
	}
	__syncthreads();
	int nsurv_before = 0;
	// A thread's rows are tid + 256 q, one after the other; the slab record of the NEXT one is requested before the results of
	// this one are stored (memory operations retire in issue order: behind the stores the next row's loads would wait for the
	// stores' acknowledgements as well).
	double nw = 0, nm[3] = {0, 0, 0}, nP[6] = {0, 0, 0, 0, 0, 0}, ncidxd = 0;
	auto request = [&](int q) {   // (no branch: a row beyond the cut, or an absorbed one, reads a line its wave reads anyway)
		const int i = min(q * 256 + tid, max(cut - 1, 0));
		const double2* row = (const double2*) (srec + (size_t) i * PRUNE_ROW);
		const double2 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3], r4 = row[4], r5 = row[5];
		nw = r0.x; nm[0] = r0.y; nm[1] = r1.x; nm[2] = r1.y;
		nP[0] = r2.x; nP[1] = r2.y; nP[2] = r3.x; nP[3] = r3.y; nP[4] = r4.x; nP[5] = r4.y;
		ncidxd = r5.x;
	};
	if (cut > 0) request(0);
	for (int q = 0; q < nchunks; q++) {
		const int  i = q * 256 + tid;
		const bool surv = survives(i);
		const unsigned long long bal = ballot64(surv);
		int base = nsurv_before;
		for (int u = 0; u < wv; u++) base += scan[q * 4 + u];
		const int total = scan[q * 4] + scan[q * 4 + 1] + scan[q * 4 + 2] + scan[q * 4 + 3];
		// (this row's slab record: the component record and, in the sixth 16 bytes, its canonical index)
		const double w = nw, Pr[6] = {nP[0], nP[1], nP[2], nP[3], nP[4], nP[5]};
		const double m0 = nm[0], m1 = nm[1], m2 = nm[2];
		const int cidx = (int) ncidxd;
		if (q + 1 < nchunks) request(q + 1);   // (uniform)
		if (surv) {
			// the reference runs on the CLR (no fused multiply-add): Merge's raw moments must round as there, or a scene far
			// from the origin loses digits of the covariance to the difference (tests: test_reweight_far_from_the_origin)
PHD_REF_ARITH
			const int pos = base + __popcll(bal & lanemask_lt());
			// Gaussian.Merge (Gaussian.cs:329-346): raw moments, the candidate first, then its set in list order
			double W = 0.0 + w;
			double M0 = 0.0 + w * m0, M1 = 0.0 + w * m1, M2 = 0.0 + w * m2;
			double C0 = 0.0 + w * (Pr[0] + m0 * m0), C1 = 0.0 + w * (Pr[1] + m0 * m1), C2 = 0.0 + w * (Pr[2] + m0 * m2);
			double C3 = 0.0 + w * (Pr[3] + m1 * m1), C4 = 0.0 + w * (Pr[4] + m1 * m2), C5 = 0.0 + w * (Pr[5] + m2 * m2);
			int nabs = 0;
			auto absorb = [&](int k) {
PHD_REF_ARITH
				nabs++;
				double wk, mk[3], Pk[6];
				load_comp(srec + (size_t) k * PRUNE_ROW, wk, mk, Pk);
				const double k0 = mk[0], k1 = mk[1], k2 = mk[2];
				W += wk;
				M0 += wk * k0; M1 += wk * k1; M2 += wk * k2;
				C0 += wk * (Pk[0] + k0 * k0); C1 += wk * (Pk[1] + k0 * k1); C2 += wk * (Pk[2] + k0 * k2);
				C3 += wk * (Pk[3] + k1 * k1); C4 += wk * (Pk[4] + k1 * k2); C5 += wk * (Pk[5] + k2 * k2);
			};
			const unsigned long long lo = nbr[2 * i], hi = nbr[2 * i + 1];
			const int cnt = (int) (lo & 0xffff);
			if (cnt <= PRUNE_NBR) {
				for (int u = 0; u < cnt; u++) {
					const int k = prune_nbr_at(lo, hi, u);
					if (owner[k] == i) absorb(k);
				}
			}
			else {
				for (int k = i + 1; k < cut; k++) {
					if (owner[k] == i) absorb(k);
				}
			}
			double ow, o0, o1, o2, oP[6];
			if (W < 1e-15) {   // Gaussian.cs:339-341
				ow = 0.0; o0 = m0; o1 = m1; o2 = m2;
				oP[0] = 1e12; oP[1] = 0; oP[2] = 0; oP[3] = 1e12; oP[4] = 0; oP[5] = 1e12;
			}
			else {
				ow = W; o0 = M0 / W; o1 = M1 / W; o2 = M2 / W;
				oP[0] = C0 / W - o0 * o0; oP[1] = C1 / W - o0 * o1; oP[2] = C2 / W - o0 * o2;
				oP[3] = C3 / W - o1 * o1; oP[4] = C4 / W - o1 * o2; oP[5] = C5 / W - o2 * o2;
			}
			const size_t ob = (size_t) p * a.cap + pos;
			{
				const double om[3] = {o0, o1, o2};
				store_comp(vout.rec + ob * MIX_REC, ow, om, oP);
			}
			a.outw[ob] = ow;   // (the weights once more as a plane: all that BestMapEstimate reads of most components)
			int covered = 0;
			if (nabs == 0 && cidx < npred && !(W < 1e-15)) {
				const double pscale = 1e-9 * fmax(fabs(Pr[0]), fmax(fabs(Pr[3]), fabs(Pr[5])));
				bool same = fabs(o0 - m0) <= 1e-9 * fabs(m0) && fabs(o1 - m1) <= 1e-9 * fabs(m1) && fabs(o2 - m2) <= 1e-9 * fabs(m2);
#pragma unroll
				for (int t = 0; t < 6; t++) same = same && fabs(oP[t] - Pr[t]) <= pscale;
				if (same) { wcopy[cidx] = ow; covered = 1; }
			}
			a.cover[ob] = covered;
		}
		nsurv_before += total;
	}
	PHD_STAMP(5);
	if (tid == 0) vout.count[p] = nsurv_before;
	PHD_STAMP_FLUSH(2, 12);
#if defined(PHD_STAMPS) && !defined(PHD_STAMP_COUNTERS)   // (the fused launch: cycles of the emit body in front of this one, slot 15)
	if (tid == 0 && a.stamps && a.stamp_kernel == 2 && tk0) a.stamps[(size_t) p * 16 + 15] = (double) (stamp_[0] - tk0);
#endif
}

#ifndef PHD_PRUNE_WAVES
#define PHD_PRUNE_WAVES 4
#endif
__global__ __launch_bounds__(256, PHD_PRUNE_WAVES) void k_prune_merge(const DevParams prm, const StepBufs a, int cutcap)
{
	extern __shared__ __align__(16) double smem[];
	prune_merge_body(prm, a, cutcap, smem);
}

// k_emit_finish and k_prune_merge as ONE launch (environment PHD_FUSE_EP=1): a particle's corrected list goes from the one
// body to the other behind a workgroup barrier, the launch boundary between two latency-bound kernels — a tail in which the
// machine drains and a ramp in which it fills — is paid once. Registers: the Kalman path compiled at this kernel's 128.
template <bool DEPTH = false>
__global__ __launch_bounds__(256, PHD_PRUNE_WAVES) void k_emit_prune(const DevParams prm, const StepBufs a, int cutcap)
{
	extern __shared__ __align__(16) double smem[];
	PHD_TL_BEGIN;
	PHD_SET_PRIO(PHD_LAT_PRIO);
#ifdef PHD_STAMPS
	const long long tk0 = clock64();
#else
	const long long tk0 = 0;
#endif
	emit_finish_body<true, false, DEPTH>(prm, a, smem);
	__syncthreads();   // (workgroup scope: what this workgroup's waves stored is visible to its loads behind the barrier)
	prune_merge_body(prm, a, cutcap, smem, tk0);
	PHD_TL_END(2);
}
