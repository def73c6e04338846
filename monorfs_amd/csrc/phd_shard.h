// phd_shard.h — the device code of the sharded step: the weights pushed to every rank, the migration plan (one workgroup,
// or a grid of them), the migrating particles packed, landed and unpacked. Included by phd_kernels.h (StepBufs, Bank,
// copy_comps) in front of phd_resample.h, whose grid resampling counts for the plan in its last launch.
#pragma once
#include "phd_device.h"

// =================================================================================================
// Sharded step: particles are sharded contiguously over ranks (one rank = one GPU: a process of its own
// with RCCL, or a shard of a phd_create_multi handle); after the global resampling a slot may need a particle that lives
// on another rank. A migrating particle travels as one fixed-size record (mig_rec_doubles).
// Everything between the global resampling kernel and the next step is decided ON THE DEVICE (k_plan_migration): the host
// never needs the source vector, only — where a collective wants split sizes (RCCL all-to-all) — 2 n counts.
// =================================================================================================

#define PLAN_GRID_MIN 8192               // (= NR_GRID_MIN: the plan's first half runs inside the grid resampling's last launch)
#define PLAN_GRID_MAXSLOTS 65536          // per-wave count arrays: 1024 global waves

struct PlanGrid {
	int* cnt;      // [n][n] records rank t takes from rank s            (this launch pair's set; NULL: no plan is counted)
	int* wcg;      // [Pg / 64] heads whose source is mine, per global wave
	int* lcg;      // [Pl / 64] heads among my own slots, per local wave
	unsigned int* used;   // [(Pl + 31) / 32] bit c: OUT slot c stays the source of a local particle
	int* bad;      // [1]
	int* cnt_next; unsigned int* used_next; int* bad_next;   // the other set: cleared by k_plan_lists
};

// the flags of slot g from its source s and the source of the slot before it (see k_plan_migration): owner rank, source rank, head
// of a run fed from another rank, malformed
__device__ __forceinline__ void plan_flags(int s, int prev, int g, int Pg, int Pl, float rPl, bool bigidx, int& t, int& sr, bool& head, bool& bad)
{
	auto rank_of = [&](int x) { return bigidx ? x / Pl : small_div(x, Pl, rPl); };
	bad = g < Pg && (s < 0 || s >= Pg || (g > 0 && prev > s));
	t = rank_of(min(g, Pg - 1));
	sr = rank_of(min(max(s, 0), Pg - 1));
	head = g < Pg && sr != t && (g == t * Pl || prev != s);
}

// ... with the sources read from the vector: this lane's, and the lane before's by a shuffle (lane 0: the word before)
__device__ __forceinline__ void plan_look(const int* __restrict__ gsrc, int g, int Pg, int Pl, float rPl, bool bigidx, int lane,
                                          int& s, int& t, int& sr, bool& head, bool& bad)
{
	s = (g < Pg) ? gsrc[g] : 0;
	int prev = __shfl_up(s, 1, 64);
	if (lane == 0) prev = (g > 0 && g < Pg) ? gsrc[g - 1] : 0;
	plan_flags(s, prev, g, Pg, Pl, rPl, bigidx, t, sr, head, bad);
}

// a flag raised on this rank, or — the gathered status words, one per lane — on any other: one trip to memory
__device__ __forceinline__ bool plan_dropped(const int* lflags, const double* gflags, int n, int lane)
{
	const int lf = *lflags;
	const double gf = (gflags && lane < n) ? gflags[lane] : 0.0;
	return lf != 0 || ballot64(gf != 0.0) != 0ull;
}

// What slot g adds to the plan's accumulators (all 64 lanes of a wave call it together; gwave: the wave's number among all slots'
// waves): the count matrix, the waves' head counts, the bitmap of OUT slots that stay a local source. Pl is a multiple of 64 — the
// host takes the one-workgroup kernel otherwise —, so a wave's slots belong to one rank.
__device__ __forceinline__ void plan_count_slot(const PlanGrid& pg, int g, int Pg, int Pl, int n, int rank, int lane, int gwave,
                                                int s, int t, int sr, bool head, bool bad)
{
	const int first = rank * Pl;
	if (bad) atomicOr(pg.bad, 1);
	if (head && !bad) atomicAdd(&pg.cnt[t * n + sr], 1);
	const unsigned long long mine = ballot64(head && !bad && sr == rank);
	if (lane == 0 && g < Pg) pg.wcg[gwave] = __popcll(mine);
	const bool myslot = g < Pg && t == rank;
	if (myslot) {
		// the heads among my own slots, per wave of them: the records' numbers (k_plan_lists)
		const unsigned long long lb = ballot64(head && !bad);
		if (lane == 0) pg.lcg[(g - first) >> 6] = __popcll(lb);
	}
	// The OUT slots that stay a local particle's source, as a bitmap. The sources never decrease, so a wave's 64 slots name a run
	// of neighbouring bits — mostly the same few: the lanes OR theirs together per word first (an atomic per slot was 2048
	// atomics on 64 words, serialised at the L2: most of the launch) and the first lane of each word's run adds it.
	const bool loc = myslot && sr == rank && !bad;
	const int word = loc ? (s - first) >> 5 : -1 - lane;   // (distinct negative numbers: no run)
	unsigned int bits = loc ? 1u << ((s - first) & 31) : 0u;
	// segmented OR over runs of equal `word` (the lanes of a run are neighbours): log steps, a lane takes what the lane `o`
	// further on holds when that lane belongs to the same word
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const int wo = __shfl_down(word, o, 64);
		const unsigned int bo = __shfl_down(bits, o, 64);
		if (lane + o < 64 && wo == word) bits |= bo;
	}
	const int wp = __shfl_up(word, 1, 64);
	if (loc && (lane == 0 || wp != word)) atomicOr(&pg.used[word], bits);
}

// The un-normalised weights of the local step, stored straight into the gathered weight vector of every destination
// (dst[t] + first): the shards of a multi-device handle write their slice into every peer's vector through peer-mapped
// pointers (the all-gather of SURVEY §5 / §8e as 16 KB of stores per peer, no copy engine, no host call per pair); the
// per-rank host hands in one destination, the buffer its collective reads. gflag: the step's status word goes along
// (slot `flagslot` behind the weights of every destination), so that a step dropped on one shard is dropped on all.
__global__ __launch_bounds__(256) void k_push_weights(const StepBufs a, double* const* dst, int ndst, int first, int flagslot)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	double* w = bank_of(a, SEL_OUT).weights;
	if (i < a.P) {
		const double v = w[i];
		for (int t = 0; t < ndst; t++) dst[t][first + i] = v;
	}
	if (i == 0 && flagslot >= 0) {
		const double f = (double) *a.flags;
		for (int t = 0; t < ndst; t++) dst[t][flagslot] = f;
	}
}

// Per-rank host: the all-gather lands as [rank][Pl + 1] — a rank's un-normalised weights and, behind them, its status word.
// The weights go to the contiguous vector the global kernel takes (gw[world Pl]), the status words behind it (gw[world Pl + r]).
__global__ __launch_bounds__(256) void k_ungather(const double* __restrict__ graw, double* __restrict__ gw, int Pl, int world)
{
	const int g = blockIdx.x * 256 + threadIdx.x, Pg = Pl * world;
	if (g < Pg) {
		const int r = g / Pl, i = g - r * Pl;
		gw[g] = graw[(size_t) r * (Pl + 1) + i];
	}
	else if (g < Pg + world) {
		const int r = g - Pg;
		gw[g] = graw[(size_t) r * (Pl + 1) + Pl];
	}
}

// The migration plan of one rank, device-resident. counts, for a world of n ranks: [0, n) records sent to rank t, [n, 2n) records
// received from rank s, then the result words MC_* (mig_word). The device plan carries the first MC_DEVICE_WORDS of them; the
// copy in pinned host memory (phd_migration_plan waits for it) also what the host would otherwise fetch, and the word it polls.
#define MC_NSEND      0   // records this rank sends
#define MC_NRECV      1   // ... and receives
#define MC_STATUS     2   // MIG_*
#define MC_RESAMPLED  3   // info[1]
#define MC_DEVICE_WORDS 4
#define MC_BEST       4   // info[0], the best particle
#define MC_FLAGS      5   // this rank's flag word
#define MC_SEQ        6   // the sequence number the host polls: written last, with release
#define PHD_MAX_DEVICES 64   // ranks of a world: the device ordinals a process may hand to phd_create / phd_create_multi
#define MIG_COUNT_WORDS (2 * PHD_MAX_DEVICES + 8)   // ints of a counts array, on the device and in pinned memory
__host__ __device__ constexpr int mig_word(int n, int k) { return 2 * n + k; }   // result word k in a world of n ranks

// One migrating particle is a record of doubles: [count | pose (7) | cap component records of MIX_REC]. A receive buffer holds
// `recvrecs` of them and, behind those, the landing flags: one 8-byte word per sending rank (k_post_landing).
#define MIG_REC_COUNT 0
#define MIG_REC_POSE  1
#define MIG_REC_COMPS 8
__host__ __device__ inline size_t mig_rec_doubles(int cap) { return (size_t) MIG_REC_COMPS + (size_t) MIX_REC * cap; }
__host__ __device__ inline size_t mig_landing_offset(int recvrecs, int cap) { return (size_t) recvrecs * mig_rec_doubles(cap); }   // in doubles
__host__ __device__ inline size_t mig_recv_doubles(int recvrecs, int cap) { return mig_landing_offset(recvrecs, cap) + PHD_MAX_DEVICES; }

#define MIG_OK        0
#define MIG_DROPPED   1   // a kernel of the step raised a flag (on this or, multi-device handle, on any shard): nothing moves
#define MIG_BAD       2   // the source vector is not a resampling result (not non-decreasing, or out of range)
#define MIG_OVERFLOW  3   // more records than the send list holds
struct MigPlan {
	int* code;         // [Pl]  per local slot: >= 0 local source slot, < 0: -(k + 1) = record k of the receive buffer
	int* fslot;        // [Pl]  OUT-bank slot record k is unpacked into (one no local particle keeps as its source)
	int* sendlist;     // [sendcap] local slots to pack, grouped by destination rank (ascending), then by destination slot
	long long* senddst;// [sendcap] destination rank << 32 | record number in that rank's receive buffer
	int* counts;       // [MIG_COUNT_WORDS] of which 2 n + MC_DEVICE_WORDS are written
	int  sendcap;
};

// exclusive prefix sum of one int per thread over the threads of the workgroup (wsum: 17 ints of LDS); *total <- the sum
__device__ __forceinline__ int block_excl_scan(int v, int* wsum, int tid, int* total)
{
	const int lane = tid & 63, wv = tid >> 6, nw = (int) (blockDim.x >> 6);
	int incl = v;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1) {
		const int y = __shfl_up(incl, o, 64);
		if (lane >= o) incl += y;
	}
	__syncthreads();   // (wsum may still be read from the scan before)
	if (lane == 63) wsum[wv] = incl;
	__syncthreads();
	int off = 0, tot = 0;
	for (int q = 0; q < nw; q++) { const int x = wsum[q]; off += (q < wv) ? x : 0; tot += x; }
	*total = tot;
	return off + incl - v;
}

// exclusive prefix, in place, over `tot` counts in LDS (more of them than threads: a chunk per thread); *total <- their sum
__device__ __forceinline__ void plan_scan_counts(int* wc, int tot, int* wsum, int tid, int nt, int* total)
{
	const int CHW = (tot + nt - 1) / nt;
	const int e0 = min(tot, tid * CHW), e1 = min(tot, e0 + CHW);
	int mysum = 0;
	for (int e = e0; e < e1; e++) mysum += wc[e];
	int run = block_excl_scan(mysum, wsum, tid, total);
	for (int e = e0; e < e1; e++) { const int x = wc[e]; wc[e] = run; run += x; }
}

// thread t < n, from the count matrix cnt[n][n] (records rank t takes from rank s): base[t] <- the first send-list position of
// destination t, roff[t] <- the record number, in destination t's receive buffer, of my first record for it
__device__ __forceinline__ void plan_offsets(const int* cnt, int n, int rank, int t, int* base, int* roff)
{
	int b = 0, r = 0;
	for (int q = 0; q < t; q++) b += (q != rank) ? cnt[q * n + rank] : 0;      // destinations before t
	for (int q = 0; q < rank; q++) r += (q != t) ? cnt[t * n + q] : 0;         // sources before me at destination t
	base[t] = b; roff[t] = r;
}

// An arriving particle is unpacked into a slot of the OUT bank that no local particle keeps as its source (at least nrecv slots
// are fed from elsewhere, so the Pl slots keep at most Pl - nrecv distinct local sources: at least nrecv slots of the OUT bank
// are free): fslot[k] <- the k-th clear bit of `used`, k < nrecv. One workgroup of nt threads; wsum: block_excl_scan's.
template <typename U>
__device__ __forceinline__ void plan_free_slots(const U* used, int Pl, int nrecv, int* fslot, int* wsum, int tid, int nt)
{
	const int words = (Pl + 31) / 32, CHW = (words + nt - 1) / nt;
	const int e0 = min(words, tid * CHW), e1 = min(words, e0 + CHW);
	auto free_bits = [&](int e) {
		unsigned int fr = ~(unsigned int) used[e];
		if (e == words - 1 && (Pl & 31)) fr &= (1u << (Pl & 31)) - 1u;
		return fr;
	};
	int nfree = 0;
	for (int e = e0; e < e1; e++) nfree += __popc(free_bits(e));
	int totfree;
	int f = block_excl_scan(nfree, wsum, tid, &totfree);
	for (int e = e0; e < e1 && f < nrecv; e++) {
		unsigned int fr = free_bits(e);
		while (fr && f < nrecv) {
			const int bit = __ffs((int) fr) - 1;
			fr &= fr - 1;
			fslot[f++] = e * 32 + bit;
		}
	}
}

// The end of a plan, by all nt threads of ONE workgroup: the counts and result words into the device plan and — hostcounts, pinned
// host memory, when the host waits for them (NULL: none) — the same words there, with what the host would otherwise fetch
// (best particle, flag word), then the sequence number it polls instead of synchronising the stream: system-scope stores, the
// fence orders every word before that one. cnt: the count matrix [n][n]; not read unless `live` (resampled, status MIG_OK).
__device__ __forceinline__ void plan_report(const MigPlan& pl, int* hostcounts, int seq, const int* cnt, int n, int rank, bool live,
                                            int nsend, int nrecv, int status, int resampled, const int* info, const int* lflags, int tid, int nt)
{
	for (int t = tid; t < n; t += nt) {
		pl.counts[t]     = (live && t != rank) ? cnt[t * n + rank] : 0;
		pl.counts[n + t] = (live && t != rank) ? cnt[rank * n + t] : 0;
	}
	if (tid == 0) {
		pl.counts[mig_word(n, MC_NSEND)] = nsend; pl.counts[mig_word(n, MC_NRECV)] = nrecv;
		pl.counts[mig_word(n, MC_STATUS)] = status; pl.counts[mig_word(n, MC_RESAMPLED)] = resampled;
	}
	if (!hostcounts) return;
	auto post = [&](int k, int v) { __hip_atomic_store(hostcounts + k, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
	for (int t = tid; t < n; t += nt) {
		post(t, (live && t != rank) ? cnt[t * n + rank] : 0);
		post(n + t, (live && t != rank) ? cnt[rank * n + t] : 0);
	}
	if (tid == 0) {
		post(mig_word(n, MC_NSEND), nsend);
		post(mig_word(n, MC_NRECV), nrecv);
		post(mig_word(n, MC_STATUS), status);
		post(mig_word(n, MC_RESAMPLED), resampled);
		post(mig_word(n, MC_BEST), info[0]);
		post(mig_word(n, MC_FLAGS), *lflags);
	}
	__threadfence_system();
	__syncthreads();
	if (tid == 0) __hip_atomic_store(hostcounts + mig_word(n, MC_SEQ), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// phd_plan_migration (phdhip.hip, the host statement of the same plan, kept as the ABI's pure function and as this kernel's
// reference in the tests) for the source vectors systematic resampling produces: those are non-decreasing (the recurrence of
// PHDNavigator.cs:731-738 only ever advances k), so "the previous slot of rank t whose source lies on rank s" is simply the
// slot before — every list is a prefix sum over flags of neighbouring slots. One workgroup of 1024 threads; every rank
// runs it on the same global vector and derives matching lists (the sender's order per destination is the receiver's order
// per source). The vector is read in rounds of 1024 consecutive slots (coalesced; the slot before comes from the
// neighbouring lane); positions in the lists are (flags before in the round's waves) + (flags before in the wave), the
// first from one scan over the per-round, per-wave counts.
//   gsrc [n Pl] global source of every slot; info[1] resampled; lflags: this rank's status word; gflags: the status words
//   of all ranks as gathered with the weights (NULL: per-rank host); hostcounts: pinned host memory the counts are
//   written to as well, followed by `seq` (the host polls that word instead of synchronising the stream); NULL: none
// LDS (ints): cnt[n][n] base[n] roff[n] wsum[20] | wc[rounds][16] send counts per round and wave | used[(Pl + 31) / 32]
//   | sg[n Pl] the source vector itself, when `staged` (it is read five times over: from LDS the rounds do not each wait
//   for a trip to memory)
#define PLAN_LDS_MAX (150 * 1024)
__host__ __device__ inline size_t plan_lds_fixed(int Pl, int n)
{
	const size_t rounds = ((size_t) Pl * n + 1023) / 1024;
	return ((size_t) n * n + 2 * n + 24 + rounds * 16 + 16 + (Pl + 31) / 32 + 4) * 4;
}
__host__ __device__ inline bool plan_staged(int Pl, int n) { return plan_lds_fixed(Pl, n) + (size_t) Pl * n * 4 <= PLAN_LDS_MAX; }
__host__ __device__ inline size_t plan_lds_bytes(int Pl, int n) { return plan_lds_fixed(Pl, n) + (plan_staged(Pl, n) ? (size_t) Pl * n * 4 : 0); }

//   gw (may be NULL): this rank's slice of the gathered (normalised, or 1 / P) weights goes back into its OUT bank here
__global__ __launch_bounds__(1024) void k_plan_migration(const int* __restrict__ gsrc, const int* __restrict__ info, const int* lflags,
                                                         const double* gflags, int Pl, int n, int rank, MigPlan pl, int* hostcounts, int seq,
                                                         const StepBufs a, const double* gw)
{
	extern __shared__ int sm[];
	const int tid = threadIdx.x, nt = (int) blockDim.x, lane = tid & 63, wv = tid >> 6;
	const int Pg = Pl * n, first = rank * Pl;
	if (gw) {
		double* wout = bank_of(a, SEL_OUT).weights;
		for (int i = tid; i < Pl; i += nt) wout[i] = gw[first + i];
	}
	const int rounds = (Pg + nt - 1) / nt, lrounds = (Pl + nt - 1) / nt;
	int* const cnt  = sm;                          // [n][n] records rank t takes from rank s
	int* const base = cnt + n * n;                 // [n] first send-list position of destination t
	int* const roff = base + n;                    // [n] record number, in destination t's receive buffer, of my first record for it
	int* const wsum = roff + n;                    // [20]
	int* const wc   = wsum + 20;                   // [rounds][16] flags per round and wave, then their exclusive prefix
	int* const used = wc + rounds * 16 + 16;       // [(Pl + 31) / 32] bit c: OUT slot c stays the source of a local particle
	int* const sg   = used + (Pl + 31) / 32 + 4;   // [Pg] the source vector (staged)
	const bool staged = plan_staged(Pl, n);
	__shared__ int s_bad;
	const float rPl = 1.0f / (float) Pl;
	bool drop = *lflags != 0;
	if (gflags) for (int t = 0; t < n; t++) drop = drop || gflags[t] != 0.0;
	const int resampled = info[1];
	int status = drop ? MIG_DROPPED : MIG_OK, nsend = 0, nrecv = 0;
	const bool bigidx = Pg >= (1 << 24);   // (the float quotient of small_div needs 24-bit operands; beyond that: the division)
	// the flags of slot g (all lanes call it; g >= Pg: none): the slot's source and the one before it from the staged vector, or from memory
	auto look = [&](int g, int& s, int& t, int& sr, bool& head, bool& bad) {
		if (!staged) { plan_look(gsrc, g, Pg, Pl, rPl, bigidx, lane, s, t, sr, head, bad); return; }
		s = (g < Pg) ? sg[g] : 0;
		plan_flags(s, (g > 0 && g < Pg) ? sg[g - 1] : 0, g, Pg, Pl, rPl, bigidx, t, sr, head, bad);
	};
	if (resampled && !drop) {   // (uniform)
		for (int i = tid; i < n * n; i += nt) cnt[i] = 0;
		for (int i = tid; i < (Pl + 31) / 32; i += nt) used[i] = 0;
		if (tid == 0) s_bad = 0;
		if (staged) {   // eight loads in flight per thread, then their stores
			for (int b0 = tid; b0 < Pg; b0 += 8 * nt) {
				int v[8];
#pragma unroll
				for (int q = 0; q < 8; q++) v[q] = (b0 + q * nt < Pg) ? gsrc[b0 + q * nt] : 0;
#pragma unroll
				for (int q = 0; q < 8; q++) if (b0 + q * nt < Pg) sg[b0 + q * nt] = v[q];
			}
		}
		__syncthreads();
		// ---- all slots: who takes a record from whom; how many records of mine every round and wave holds
		bool anybad = false;
		for (int r = 0; r < rounds; r++) {
			const int g = r * nt + tid;
			int s, t, sr;
			bool head, bad;
			look(g, s, t, sr, head, bad);
			anybad = anybad || bad;
			if (head && !bad) atomicAdd(&cnt[t * n + sr], 1);
			const unsigned long long mine = ballot64(head && !bad && sr == rank);
			if (lane == 0) wc[r * 16 + wv] = __popcll(mine);
		}
		if (anybad) s_bad = 1;
		__syncthreads();
		plan_scan_counts(wc, rounds * 16, wsum, tid, nt, &nsend);   // the (round, wave) counts, in slot order
		if (tid < n) plan_offsets(cnt, n, rank, tid, base, roff);
		__syncthreads();
		if (s_bad) status = MIG_BAD;
		else if (nsend > pl.sendcap) status = MIG_OVERFLOW;
		if (status == MIG_OK) {
			// ---- my send list: the heads among other ranks' slots whose source is mine, in slot order (= by destination, then slot)
			for (int r = 0; r < rounds; r++) {
				const int g = r * nt + tid;
				int s, t, sr;
				bool head, bad;
				look(g, s, t, sr, head, bad);
				const bool mine = head && sr == rank;
				const unsigned long long bal = ballot64(mine);
				if (mine) {
					const int k = wc[r * 16 + wv] + __popcll(bal & lanemask_lt());
					pl.sendlist[k] = s - first;
					pl.senddst[k] = ((long long) t << 32) | (long long) (roff[t] + (k - base[t]));
				}
			}
			// ---- my slots: local source, or the record that feeds the run the slot belongs to (records numbered in slot order:
			// with non-decreasing sources that is the order "by source rank, then by slot" the sender packs them in)
			__syncthreads();   // (wc is reused)
			for (int r = 0; r < lrounds; r++) {
				const int i = r * nt + tid;
				int s, t, sr;
				bool head, bad;
				look(i < Pl ? first + i : Pg, s, t, sr, head, bad);
				const unsigned long long bal = ballot64(head);
				if (lane == 0) wc[r * 16 + wv] = __popcll(bal);
			}
			__syncthreads();
			plan_scan_counts(wc, lrounds * 16, wsum, tid, nt, &nrecv);
			__syncthreads();
			for (int r = 0; r < lrounds; r++) {
				const int i = r * nt + tid;
				int s, t, sr;
				bool head, bad;
				look(i < Pl ? first + i : Pg, s, t, sr, head, bad);
				const unsigned long long bal = ballot64(head);
				if (i < Pl) {
					if (sr == rank) {
						pl.code[i] = s - first;
						atomicOr(&used[(s - first) >> 5], 1 << ((s - first) & 31));
					}
					else {
						// heads up to and including this slot: the number of the record that feeds it (a slot inside a run
						// carries the count of its run's head: no head lies in between)
						const int slot = wc[r * 16 + wv] + __popcll(bal & (lanemask_lt() | (1ull << lane)));
						pl.code[i] = -slot;   // record slot - 1
					}
				}
			}
			__syncthreads();
			plan_free_slots(used, Pl, nrecv, pl.fslot, wsum, tid, nt);
		}
		else { nsend = 0; nrecv = 0; }
	}
	__syncthreads();
	plan_report(pl, hostcounts, seq, cnt, n, rank, resampled && status == MIG_OK, nsend, nrecv, status, resampled, info, lflags, tid, nt);
}

// =================================================================================================================================
// The same plan over a GRID of workgroups (round 5), for global vectors of PLAN_GRID_MIN slots and more: one workgroup of 1024
// threads took 34 us for the five passes over an 8 x 2048 vector — instruction-bound on ONE compute unit, on every rank, in
// every resampling step. Here every thread owns one slot of the global vector and two launches do the work:
//   k_plan_count   every slot: is it the head of a run that needs a record (flags of neighbouring slots, as above)? The n x n
//                  count matrix by atomics (only heads add: a few hundred), per wave the heads whose source is MINE (the send
//                  list's order) and, over this rank's own slots, the heads at all (the record numbers) and the bitmap of OUT
//                  slots that stay a local particle's source
//   k_plan_lists   positions = (counts of the waves before) + (heads before in the wave): the send list with each record's
//                  destination and number, the code of every local slot; one workgroup lays the arrivals' free slots out and
//                  writes the counts (to the host too, when it waits for them)
// Two sets of the accumulators alternate between launches: k_plan_lists clears the set the NEXT pair of launches adds to, so
// that no launch — and no memset on the stream — stands between the resampling kernel and k_plan_count.
__global__ __launch_bounds__(256) void k_plan_count(const int* __restrict__ gsrc, const int* __restrict__ info, const int* lflags,
                                                    const double* gflags, int Pl, int n, int rank, PlanGrid pg)
{
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int Pg = Pl * n, g = blockIdx.x * 256 + tid;
	int s, t, sr;
	bool head, bad;
	const bool bigidx = Pg >= (1 << 24);
	plan_look(gsrc, g, Pg, Pl, 1.0f / (float) Pl, bigidx, lane, s, t, sr, head, bad);   // (its loads are in flight while the status words arrive)
	const int resampled = info[1];
	const bool drop = plan_dropped(lflags, gflags, n, lane);
	if (drop || !resampled) return;   // dropped, or not resampled: nothing moves (k_plan_lists writes the status)
	plan_count_slot(pg, g, Pg, Pl, n, rank, lane, blockIdx.x * 4 + wv, s, t, sr, head, bad);
}

//   gw (may be NULL): this rank's slice of the gathered (normalised, or 1 / P) weights goes back into its OUT bank here
__global__ __launch_bounds__(256) void k_plan_lists(const int* __restrict__ gsrc, const int* __restrict__ info, const int* lflags,
                                                    const double* gflags, int Pl, int n, int rank, MigPlan pl, PlanGrid pg, int* hostcounts, int seq,
                                                    const StepBufs a, const double* gw)
{
	__shared__ int s_cnt[PHD_MAX_DEVICES * PHD_MAX_DEVICES], s_base[PHD_MAX_DEVICES], s_roff[PHD_MAX_DEVICES], s_w[20], s_ns, s_nr;
	const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const int Pg = Pl * n, first = rank * Pl, g = blockIdx.x * 256 + tid;
	int s, t, sr;
	bool head, bad;
	const bool bigidx = Pg >= (1 << 24);
	plan_look(gsrc, g, Pg, Pl, 1.0f / (float) Pl, bigidx, lane, s, t, sr, head, bad);
	// Everything this launch reads of the counting's results is requested up front, together — the count matrix into LDS, the
	// waves' counts into registers — and only then looked at: every dependent trip to memory is a microsecond here.
	const int resampled = info[1], badword = pg.bad[0];
	const bool drop = plan_dropped(lflags, gflags, n, lane);
	if (gw && g >= first && g < first + Pl) bank_of(a, SEL_OUT).weights[g - first] = gw[g];   // this rank's slice of the weights
	// the accumulators of the NEXT pair of launches (the set the pair before this one added to): cleared whatever this step does —
	// the host alternates the sets with every pair, and a set left as a resampling step filled it would be met again two pairs on
	{
		const int gt = blockIdx.x * 256 + tid, gn = gridDim.x * 256;
		for (int q = gt; q < n * n; q += gn) pg.cnt_next[q] = 0;
		for (int q = gt; q < (Pl + 31) / 32; q += gn) pg.used_next[q] = 0u;
		if (gt == 0) pg.bad_next[0] = 0;
	}
	if (!resampled || drop) {
		// Nothing was counted (the counting returns at the same test) and nothing moves: the step's most common end on a frame
		// that does not deplete the particle set. One workgroup writes the status; this pair's set of accumulators is still clear.
		if (blockIdx.x == 0) plan_report(pl, hostcounts, seq, nullptr, n, rank, false, 0, 0, drop ? MIG_DROPPED : MIG_OK, resampled, info, lflags, tid, 256);
		return;
	}
	int cv[16];
#pragma unroll
	for (int q = 0; q < 16; q++) cv[q] = (tid + 256 * q < n * n) ? pg.cnt[tid + 256 * q] : 0;
	const int gwv = blockIdx.x * 4 + wv;                 // this wave's number among all slots' waves (at most 1024)
	const bool myslots = g < Pg && t == rank;            // (wave-uniform: Pl is a multiple of 64)
	const int lw = myslots ? (g - first) >> 6 : 0;       // ... and among my own slots' waves
	int wq[16], lq[16];
#pragma unroll
	for (int q = 0; q < 16; q++) {
		wq[q] = (lane + 64 * q < gwv) ? pg.wcg[lane + 64 * q] : 0;
		lq[q] = (lane + 64 * q < lw) ? pg.lcg[lane + 64 * q] : 0;
	}
#pragma unroll
	for (int q = 0; q < 16; q++) if (tid + 256 * q < n * n) s_cnt[tid + 256 * q] = cv[q];
	__syncthreads();
	if (tid < n) plan_offsets(s_cnt, n, rank, tid, s_base, s_roff);
	if (wv == 0) {
		int ns = (lane < n && lane != rank) ? s_cnt[lane * n + rank] : 0, nr_ = (lane < n && lane != rank) ? s_cnt[rank * n + lane] : 0;
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) { ns += __shfl_xor(ns, o, 64); nr_ += __shfl_xor(nr_, o, 64); }
		if (lane == 0) { s_ns = ns; s_nr = nr_; }
	}
	__syncthreads();
	int status = drop ? MIG_DROPPED : MIG_OK, nsend = 0, nrecv = 0;
	if (resampled && !drop) {
		if (badword) status = MIG_BAD;
		nsend = s_ns; nrecv = s_nr;
		if (status == MIG_OK && nsend > pl.sendcap) status = MIG_OVERFLOW;
	}
	const bool live = resampled && status == MIG_OK;
	if (live) {
		// heads of mine in the waves before this one; heads among my slots in the local waves before
		int acc = 0, lacc = 0;
#pragma unroll
		for (int q = 0; q < 16; q++) { acc += wq[q]; lacc += lq[q]; }
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) { acc += __shfl_xor(acc, o, 64); lacc += __shfl_xor(lacc, o, 64); }
		const bool mine = head && sr == rank;
		const unsigned long long bal = ballot64(mine);
		if (mine) {
			const int k = acc + __popcll(bal & lanemask_lt());
			pl.sendlist[k] = s - first;
			pl.senddst[k] = ((long long) t << 32) | (long long) (s_roff[t] + (k - s_base[t]));
		}
		if (myslots) {   // (wave-uniform)
			const int i = g - first;
			// heads up to and including this slot, among my slots: the number of the record that feeds it (a slot inside a run
			// carries the count of its run's head: no head lies in between)
			const unsigned long long hb = ballot64(head);
			if (sr == rank) pl.code[i] = s - first;
			else pl.code[i] = -(lacc + __popcll(hb & (lanemask_lt() | (1ull << lane))));   // record (that count) - 1
		}
	}
	if (blockIdx.x != 0) return;
	// ---- one workgroup: the arrivals' free slots, the counts
	if (live) plan_free_slots(pg.used, Pl, nrecv, pl.fslot, s_w, tid, 256);
	else { nsend = 0; nrecv = 0; }
	plan_report(pl, hostcounts, seq, s_cnt, n, rank, live, nsend, nrecv, status, resampled, info, lflags, tid, 256);
}

// Pack the particles other ranks take: record k of the send list = particle sendlist[k] of the OUT bank. sendbuf != NULL:
// the records go, in list order, into this rank's send buffer (the host's all-to-all moves them); NULL: each record is
// stored straight into its place in the destination's receive buffer (recvbase[t], a peer-mapped pointer: multi-device
// handle). The count comes from the device plan: a fixed grid strides over the records.
__global__ __launch_bounds__(256) void k_pack_particles(const StepBufs a, const MigPlan pl, int n, double* sendbuf, double* const* recvbase)
{
	const int tid = threadIdx.x;
	const int nsend = pl.counts[mig_word(n, MC_NSEND)];
	if (pl.counts[mig_word(n, MC_STATUS)] != MIG_OK) return;
	const MixView from = bank_view(a, SEL_OUT);
	const Bank bo = bank_of(a, SEL_OUT);
	const size_t rec = mig_rec_doubles(a.cap);
	for (int r = blockIdx.x; r < nsend; r += gridDim.x) {
		const int s = pl.sendlist[r];
		double* o;
		if (sendbuf) o = sendbuf + (size_t) r * rec;
		else {
			const long long d = pl.senddst[r];
			o = recvbase[(int) (d >> 32)] + (size_t) (d & 0xffffffffll) * rec;
		}
		const int nc = from.count[s];
		if (tid == 0) o[MIG_REC_COUNT] = (double) nc;
		if (tid < 7) o[MIG_REC_POSE + tid] = bo.poses[(size_t) s * 7 + tid];
		copy_comps(o + MIG_REC_COMPS, from.rec + (size_t) s * a.cap * MIX_REC, nc, tid, 256);
	}
}

// The landing flags (round 5): behind k_pack_particles on the sender's stream, one wave stores the step's number into word
// `rank` of the flag area at the end of EVERY peer's receive buffer (fine-grained memory, system-scope release: this launch
// begins when the pack kernel — its peer stores with it — has ended, and the fence orders whatever is still in flight
// before the flag). The receiver's k_wait_landing waits for the words of the ranks it takes records from: the
// one-word all-reduce that played landing barrier until round 4 is a second collective the step does not need.
__global__ __launch_bounds__(64) void k_post_landing(double* const* recvbase, int n, int rank, size_t flagoff, unsigned long long seq)
{
	const int t = threadIdx.x;
	__threadfence_system();
	if (t < n && t != rank) {
		unsigned long long* w = (unsigned long long*) (recvbase[t] + flagoff) + rank;
		__hip_atomic_store(w, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
	}
}

// The receiver's wait as ONE wave in front of k_finish_sharded (the default): lane t polls the word of rank t when this step
// takes records from it; the launch boundary behind it is the acquire for everything k_finish_sharded reads. (The same loop inside
// k_finish_sharded saved that boundary, ~3 us, but a grid that waits holds every slot of the device for as long as it waits: a
// standstill when ranks share one GPU. DESIGN §6.) Bounded: landing_ticks of the 100 MHz counter, then PHD_FLAG_ORDER_TIMEOUT — a
// peer that never posts has died.
__global__ __launch_bounds__(64) void k_wait_landing(const MigPlan pl, int n, const unsigned long long* landing, unsigned long long seq,
                                                     long long landing_ticks, int* flags)
{
	const int tid = threadIdx.x;
	const int nrecv = pl.counts[mig_word(n, MC_NRECV)], status = pl.counts[mig_word(n, MC_STATUS)], resampled = pl.counts[mig_word(n, MC_RESAMPLED)];
	if (status != MIG_OK || !resampled || nrecv <= 0) return;
	if (tid < n && pl.counts[n + tid] > 0) {
		const long long t0 = wall_clock64();
		while ((long long) (__hip_atomic_load(landing + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) - seq) < 0) {
			if (wall_clock64() - t0 > landing_ticks) { atomicOr(flags, PHD_FLAG_ORDER_TIMEOUT); break; }
			__builtin_amdgcn_s_sleep(8);
		}
	}
	__threadfence_system();
}

// End of a sharded step, one workgroup per local particle; what it does is read from the device plan, not decided by the
// host. The roles are those of the single-handle step (next_roles / keep_roles, phd_kernels.h):
//   dropped step (the plan's status is not MIG_OK): keep_roles
//   not resampled: slots identity
//   resampled: as in the single-handle step no local mixture is copied — particle i whose source is a local particle reads
//     that particle's slot of the OUT bank from now on; a particle that arrives from another rank (record j of the receive
//     buffer) is unpacked into a slot of the OUT bank that no local particle uses as a source (fslot[j]) and read from
//     there. Block b unpacks record b (if there is one) and sets up particle b: small arrays into TMP, slot into inslot.
//   frozen: the slots of the result go to `slots` only
//   (with landing flags, k_wait_landing in front of this launch has seen the records of the receive buffer arrive)
__global__ __launch_bounds__(256) void k_finish_sharded(const StepBufs a, const MigPlan pl, int n, const double* recvbuf, double weight,
                                                        int* sel_next, int frozen, int* inslot, int* slots)
{
	const int i = blockIdx.x, tid = threadIdx.x;
	const int nrecv = pl.counts[mig_word(n, MC_NRECV)], status = pl.counts[mig_word(n, MC_STATUS)], resampled = pl.counts[mig_word(n, MC_RESAMPLED)];
	const BankRoles now = roles_now(a.sel);   // (requested with the plan's words above)
	if (status != MIG_OK) {
		if (i == 0) keep_roles(a.sel, sel_next, tid);
		return;
	}
	if (i == 0 && tid == 0) next_roles(now, sel_next, resampled, frozen);
	if (!resampled) {
		if (tid == 0) {
			slots[i] = i;
			if (!frozen) inslot[i] = i;
		}
		return;
	}
	const size_t rec = mig_rec_doubles(a.cap);
	if (i < nrecv) {
		const MixView dst = bank_view(a, SEL_OUT);
		const double* r = recvbuf + (size_t) i * rec;
		const int nc = min(max((int) r[MIG_REC_COUNT], 0), a.cap);   // (a record is what a peer packed; never trust a count with a store loop)
		const size_t db = (size_t) pl.fslot[i] * a.cap;
		copy_comps(dst.rec + db * MIX_REC, r + MIG_REC_COMPS, nc, tid, 256);
	}
	const Bank bo = bank_of(a, SEL_OUT), bt = bank_of(a, SEL_TMP);
	const int code = pl.code[i];
	int slot;
	if (code >= 0) {
		slot = code;
		if (tid == 0) bt.count[i] = bo.count[code];
		if (tid < 7) bt.poses[(size_t) i * 7 + tid] = bo.poses[(size_t) code * 7 + tid];
	}
	else {
		const int j = -(code + 1);
		const double* r = recvbuf + (size_t) j * rec;
		slot = pl.fslot[j];
		if (tid == 0) bt.count[i] = min(max((int) r[MIG_REC_COUNT], 0), a.cap);
		if (tid < 7) bt.poses[(size_t) i * 7 + tid] = r[MIG_REC_POSE + tid];
	}
	if (tid == 0) {
		bt.weights[i] = weight;
		slots[i] = slot;
		if (!frozen) inslot[i] = slot;
	}
}
