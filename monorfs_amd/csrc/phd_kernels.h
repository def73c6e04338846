// phd_kernels.h — hand-written HIP kernels (gfx950, wave64) of the RB-PHD-SLAM inner loop.
//
// One workgroup per particle everywhere (particles are independent through predict / correct /
// prune / reweight: PHDNavigator.cs:326-339). Mixtures live in HBM as ONE 80-byte record per component
// (w, mean x/y/z, covariance xx/xy/xz/yy/yz/zz), [particle][slot][10] doubles (round 4; ten planes before): a
// wavefront that reads 64 consecutive components of a particle reads 5 KB of whole lines with five 16-byte loads per
// lane, and a component picked by index (the gathers of k_prune_merge, the queued pairs of k_emit_finish, the picks of
// BestMapEstimate) costs two 64-byte sectors instead of ten.
//
//   k_sweep (phd_sweep.h), k_emit_finish (phd_correct.h) : PredictConditional + CorrectConditional
//                       (+ the MinWeight cut of PruneModel)
//   k_prune_merge     : PruneModel (sort by weight, MaxQuantity cap, greedy merge)
//   k_weight_alpha    : WeightAlpha = BestMapEstimate + mixture densities + SetLogLikelihood
//   k_normalise_resample, k_gather_particles : particle weights, BestParticle, systematic resampling
#pragma once
#include "phd_device.h"

// status bits written by the kernels into StepBufs::flags
#define PHD_FLAG_EMIT_OVERFLOW   1   // corrected components did not fit emit_capacity
#define PHD_FLAG_J_OVERFLOW      2   // map estimate larger than the landmark scratch
#define PHD_FLAG_BIG_CLUSTER     4   // association cluster beyond the on-device solver's cap
#define PHD_FLAG_ORDER_TIMEOUT   8   // a wait on the device gave up: a helper workgroup of k_particle_chain for its main, or k_wait_landing for a peer's landing flag

#define MIX_REC 10   // doubles per component record: w, m[3], P[6] (upper triangle)

struct MixView {
	double* rec;      // component i of the bank (particle slot s, index c: i = s * cap + c) at rec + i * MIX_REC
	int*    count;
};

// a component record in and out of registers: five 16-byte accesses (records are 80 bytes apart, 16-byte aligned)
__device__ __forceinline__ void load_comp(const double* __restrict__ r, double& w, double m[3], double P[6])
{
	const double2* q = (const double2*) r;
	const double2 a = q[0], b = q[1], c = q[2], d = q[3], e = q[4];
	w = a.x; m[0] = a.y; m[1] = b.x; m[2] = b.y;
	P[0] = c.x; P[1] = c.y; P[2] = d.x; P[3] = d.y; P[4] = e.x; P[5] = e.y;
}

__device__ __forceinline__ void store_comp(double* __restrict__ r, double w, const double m[3], const double P[6])
{
	double2* q = (double2*) r;
	q[0] = make_double2(w, m[0]);
	q[1] = make_double2(m[1], m[2]);
	q[2] = make_double2(P[0], P[1]);
	q[3] = make_double2(P[2], P[3]);
	q[4] = make_double2(P[4], P[5]);
}

// `n` whole records from one place to another by the threads of the workgroup (16 bytes per thread and trip: whole lines)
__device__ __forceinline__ void copy_comps(double* __restrict__ dst, const double* __restrict__ src, int n, int tid, int nthreads)
{
	double2* d = (double2*) dst;
	const double2* s = (const double2*) src;
	for (int i = tid; i < n * (MIX_REC / 2); i += nthreads) d[i] = s[i];
}

// one of the three state banks: mixture records [Pcap][cap][10], counts, poses, weights
struct Bank {
	double* mix;
	int*    count;
	double* poses;    // [Pcap][7]
	double* weights;  // [Pcap]
};

// Roles of the three banks. A bank holds the mixture records of all particles and their small arrays (count, pose,
// weight). Resampling does not copy mixtures: after it the small arrays of the new particles sit in one bank (SEL_IN)
// while their mixtures are still the ones the step wrote into another (SEL_INMIX), particle p's at slot inslot[p]
// (the deep copies of PHDNavigator.cs:740-741 are what an indirection makes of them). OUT differs from IN and INMIX;
// TMP differs from IN and OUT (it may be INMIX: only its small arrays are written).
#define SEL_IN     0   // bank whose small arrays a step reads
#define SEL_OUT    1   // bank a step writes
#define SEL_TMP    2   // bank the small arrays of a resampled state go to
#define SEL_RES    3   // bank holding the small arrays of the last step's result
#define SEL_INMIX  4   // bank whose mixtures a step reads, through inslot
#define SEL_RESMIX 5   // bank holding the mixtures of the last step's result (slots: the resampling sources)
#define SEL_STRIDE 8

// The roles of the next step, decided on the device at the end of a step — the single-handle one (rotate_roles, k_nr_slots,
// k_nr_sources in phd_resample.h) and the sharded one (k_finish_sharded, phd_shard.h) alike, so the host never waits inside a
// step and a single handle and the ranks of a sharded run rotate the same way. No mixture is copied:
//   not resampled: the new state is the OUT bank                      -> (IN, OUT, TMP, INMIX) = (O, I, T, O), slots identity
//   resampled    : small arrays of particle i <- OUT[src[i]] into TMP -> (IN, OUT, TMP, INMIX) = (T, I, O, O), slots src
//   frozen       : roles and slots stay (benchmark steady state); RES / RESMIX say where the result is (slots: src)
// BankRoles: the roles of this step as its kernels read them (with whatever else they load first: one trip to memory).
struct BankRoles { int in, out, tmp, inmix; };

__device__ __forceinline__ BankRoles roles_now(const int* sel) { return BankRoles{sel[SEL_IN], sel[SEL_OUT], sel[SEL_TMP], sel[SEL_INMIX]}; }

// (one thread of the launch)
__device__ __forceinline__ void next_roles(const BankRoles& r, int* sel_next, int resampled, int frozen)
{
	const int I = r.in, O = r.out, T = r.tmp, X = r.inmix;
	if (frozen)         { sel_next[SEL_IN] = I; sel_next[SEL_OUT] = O; sel_next[SEL_TMP] = T; sel_next[SEL_INMIX] = X; }
	else if (resampled) { sel_next[SEL_IN] = T; sel_next[SEL_OUT] = I; sel_next[SEL_TMP] = O; sel_next[SEL_INMIX] = O; }
	else                { sel_next[SEL_IN] = O; sel_next[SEL_OUT] = I; sel_next[SEL_TMP] = T; sel_next[SEL_INMIX] = O; }
	sel_next[SEL_RES]    = resampled ? T : O;
	sel_next[SEL_RESMIX] = O;
}

// A kernel of the step raised a flag (emit capacity, landmark scratch; a failed migration): what it wrote into the OUT bank is
// not a valid state. The step is dropped as a whole — the roles stay, nothing of the current state was touched — and the host
// finds the flag at its next phd_sync. (The first SEL_STRIDE threads of one workgroup.)
__device__ __forceinline__ void keep_roles(const int* sel, int* sel_next, int tid)
{
	if (tid < SEL_STRIDE) sel_next[tid] = sel[tid];
}

struct StepBufs {
	int P;          // particles of this handle
	int p0;         // first particle of this launch (a step may be split into sub-ranges on concurrent streams)
	int cap;        // slots per particle in a mixture slab
	int M;          // measurements
	int Mcap;       // stride of per-measurement scratch
	int ecap;       // emit scratch slots per particle
	int Jcap;       // landmark scratch per particle
	Bank bank[3];
	const int* sel; // [SEL_STRIDE] device-resident roles of the banks for this step (no host round trip to rotate them)
	const int* inslot;   // [P] slot of particle p's mixture in the INMIX bank
	const double* z;         // [M][3]
	// corrected-but-unpruned components (weight >= MinWeight; in a step: those at or above the cut floor, see emit_all), unsorted
	double* emit_w;      // [P][ecap]
	int*    emit_idx;    // [P][ecap] canonical position in the reference's `corrected` list
	double* emit_rec;    // [P][ecap][10] the detection updates as component records (w, mean, covariance upper triangle); not written for the misdetection copies
	int*    emit_count;  // [P]
	// births of the predict step
	int*    born_count;  // [P]
	int*    born_k;      // [P][Mcap]
	double* born_mean;   // [P][Mcap][3]
	// reweight outputs
	double* alpha;       // [P]
	double* setll;       // [P]
	int*    flags;       // [1]
	struct MurtyNodes* murty;   // [P] workspace of the big-cluster solver (clusters of 6 .. 64 rows)
	char*   bigws;       // association slab: workspaces of the clusters beyond 64 rows, handed out by a bump counter
	unsigned long long  bigws_bytes;
	unsigned long long* bigws_used;   // reset at the end of every step (k_normalise_resample) / by the host behind a stage launch; a quasi batch brings its own
	double* jscratch;    // [P] landmark-indexed arrays of k_weight_alpha when the map estimate outgrows LDS
	// (component, measurement) pairs that may reach MinWeight, queued by k_sweep for k_emit_finish
	int*    cand;        // [P][candcap]
	int     candcap;
	int*    cand_count;  // [P][4] entries in each wave's segment of the queue (above candcap / 4: it overflowed)
	double* denom;       // [P][Mcap] kappa + weightsum[z]
	double* srec;        // [P][cutcap][12] k_prune_merge: the kept records in sorted order (component record, canonical index, spare)
	double* outw;        // [P][cap] the weights of the pruned mixture once more, as a plane of their own (k_prune_merge -> BestMapEstimate of k_alpha_assoc, which reads nothing else of most components)
	// map estimate handed from k_alpha_assoc to k_alpha_density
	double* alm;         // [P][3][Jcap] landmark means
	int*    aJ;          // [P] landmarks
	double* account;     // [P] expected size of the corrected map
	// QuasiSetLogLikelihood batches (k_quasi_setll): candidate poses, the landmark set, its size
	const double* qposes;   // [P][7]
	const double* qlm;      // [qJ][3]
	int     qJ;
	double* qgrad;       // [P][6] pose gradients (k_quasi_setll_grad)
	int     qavg;        // TemperedAverage normalisation: 0 as the source reads, 1 weights / their sum
	double* wcopy;       // [P][cap + Mcap] weight of the surviving misdetection copy of predicted component c (0: none), k_prune_merge -> k_alpha_density
	int*    cover;       // [P][cap] 1: this pruned component is such a copy
	double* stamps;      // [P][16] phase stamps of the diagnostic build (NULL otherwise)
	double* ratio;       // [P] the density part of log alpha, left by whichever of a particle's two workgroups in k_particle_chain has it (alpha_meet)
	int     all_pairs;   // 1: k_sweep evaluates every (component, measurement) pair, the radius gate only masks (SURVEY §8d's benchmark
	                     // mode: the unit count P C M is exact); 0: a visit whose 64 pairs all lie outside the gate is skipped
	int     emit_all;    // 1 (phd_stage_run alone): the emit body writes every corrected component that reaches MinWeight; 0 (every step): it may leave
	                     // out detection updates that cannot survive the MaxQuantity cut of the prune behind it (the cut floor, phd_correct.h)
	int     stamp_kernel; // which kernel writes them (env PHD_STAMP_KERNEL): 2 prune, 3 assoc, 4 density, 1 correct, 5 the one-launch chain
	// k_particle_chain with a HELPER workgroup per particle for the densities of WeightAlpha (two workgroups per particle for that body)
	int           dsplit;   // 1: the launch has 2 P workgroups, the second P are the helpers (2 - 4: test and measuring switches, PHD_DSPLIT_LATE)
	unsigned int  dstamp;   // this launch's number (never 0, grows by one per launch of the chain): what the words below are compared with
	unsigned int* dsync;    // [P][3]: helper ready (16 dstamp + its XCD) | the main's word (2 dstamp + {0 it keeps the density sums, 1 the helper runs them}) | ticket (alpha_meet)
};

// The bank playing `role`. The roles rotate on the device (a.sel lives in device memory), so the index is not known
// at launch; choosing among the three kernel-argument entries by comparison keeps them in scalar registers — indexing
// the array dynamically makes the compiler copy the argument block to scratch memory.
__device__ __forceinline__ Bank bank_of(const StepBufs& a, int role)
{
	const int s = a.sel[role];
	Bank b;
	b.mix     = (s == 0) ? a.bank[0].mix     : ((s == 1) ? a.bank[1].mix     : a.bank[2].mix);
	b.count   = (s == 0) ? a.bank[0].count   : ((s == 1) ? a.bank[1].count   : a.bank[2].count);
	b.poses   = (s == 0) ? a.bank[0].poses   : ((s == 1) ? a.bank[1].poses   : a.bank[2].poses);
	b.weights = (s == 0) ? a.bank[0].weights : ((s == 1) ? a.bank[1].weights : a.bank[2].weights);
	return b;
}

// The mixtures of the bank playing `role` and the counts that go with them. For SEL_IN the records are those of the
// INMIX bank: particle p's components start at in_base(a, p), its count is count[p].
__device__ __forceinline__ MixView bank_view(const StepBufs& a, int role)
{
	const Bank b = bank_of(a, role);
	const double* mix = (role == SEL_IN) ? bank_of(a, SEL_INMIX).mix : b.mix;
	MixView v;
	v.rec = const_cast<double*>(mix);
	v.count = b.count;
	return v;
}

__device__ __forceinline__ size_t in_base(const StepBufs& a, int p) { return (size_t) a.inslot[p] * a.cap; }

#define TILE 256   // components staged per LDS tile

#include "phd_correct.h"

// (PHD_ONLY_EP: a translation unit of k_emit_finish / k_prune_merge / k_emit_prune alone — scripts/kres.sh compiles it in seconds
// to read one kernel's registers and scratch while it is being worked on; never the product build)
#ifndef PHD_ONLY_EP
#include "phd_sweep.h"
#endif

#include "phd_prune.h"

#ifndef PHD_ONLY_EP
#include "phd_alpha.h"

#include "phd_shard.h"
#include "phd_resample.h"

#ifndef PHD_HELPER_PRIO
#define PHD_HELPER_PRIO 3   // s_setprio of the chain's helper workgroups while they run the density sums
#endif

// The per-particle chain of a step as ONE launch, for small particle sets (the real-time regime of the reference: 20 - 800
// particles at 30 Hz, plots/scripts/chap3/S4-particles.sh:14-15; BASELINE config A): a particle's predict / correct / prune /
// reweight touch nothing of another particle, so its workgroup runs the five kernels' bodies back to back, with a
// workgroup barrier where a launch boundary was, all of them in ONE LDS pool (the largest of their layouts,
// chain_lds_bytes: ~38 KB). With at most two workgroups per CU the kernels were latency-bound launches of 8 - 30 us each
// with a ramp and a tail; here there are no boundaries until the particle weights meet in k_normalise_resample, and
// registers to spare (245). On a full machine (2048 particles) a 128-register build of it at four workgroups per CU
// measured 0.785 ms per step against 0.71 for the separate kernels on two streams: not used there.
template <int ZB>
__host__ __device__ inline int chain_lds_bytes(int cutcap)
{
	int d = SweepLds<ZB>::doubles;
	if (EMIT_LDS_DOUBLES > d) d = EMIT_LDS_DOUBLES;
	if (DENS_LDS_DOUBLES > d) d = DENS_LDS_DOUBLES;
	int b = d * 8;
	const int pb = prune_lds(cutcap).bytes, ab = alpha_lds(ZB * 64, cutcap).bytes;
	if (pb > b) b = pb;
	if (ab > b) b = ab;
	return b;
}

template <int ZB, bool HALF = false, bool DEPTH = false>
__global__ __launch_bounds__(256, 1) void k_particle_chain(const DevParams prm, const StepBufs a, int cutcap, int with_alpha)
{
	extern __shared__ __align__(16) double smem[];
	// Two workgroups per particle where the chain allows it (a.dsplit: the launch has 2 nmain workgroups): WeightAlpha's density sums
	// (alpha_density_body) need the pruned map and the map estimate, not the association — so the HELPER of particle p, workgroup
	// nmain + p, runs them BESIDE the main workgroup's association instead of behind it. The helper says it is there (the launch's
	// number and its XCD) and waits for the main's word; the MAIN never waits: where its map estimate is final (alpha_assoc_body)
	// it looks whether its helper has reported from the same XCD and hands the sums over, or keeps them — the same body, the same
	// bits either way. The two meet in alpha_meet. A helper only ever waits for a workgroup that was handed out before it, and
	// gives up (step dropped: a.flags) after 2 s of the 100 MHz counter.
	const int nmain = a.dsplit ? (int) (gridDim.x >> 1) : (int) gridDim.x;
	if (a.dsplit && (int) blockIdx.x >= nmain) {
		// (whose helper: workgroups go to the XCDs in turn, workgroup b to XCD b mod 8, so helper h = b - nmain takes, within its group of
		// eight particles, the one whose main workgroup has b's residue — with a particle count that is no multiple of 8 the helpers
		// would otherwise all sit on another XCD than their mains and never be picked; the last, incomplete group stays as it is)
		const int h = (int) blockIdx.x - nmain;
		const int p = a.p0 + (((h | 7) < nmain) ? (h & ~7) + ((h + nmain) & 7) : h);
		__shared__ int s_go[1];
		if (!with_alpha || a.dsplit == 3) return;   // (3: a measuring switch — helpers that leave at once)
		// (while it waits: what the density sums can have ready from the prior mixture alone)
		const double pre_pcount = alpha_density_prestage(a, smem, p);
		if (threadIdx.x == 0) {
			unsigned int* w = a.dsync + 3 * (size_t) p;
			if (a.dsplit == 2) {   // (test switch PHD_DSPLIT_LATE=1: a helper that reports 0.5 ms late — every main keeps its sums)
				const long long t1 = wall_clock64();
				while (wall_clock64() - t1 < 50000LL) __builtin_amdgcn_s_sleep(64);
			}
			__hip_atomic_store(w, (a.dstamp << 4) | (a.dsplit == 4 ? 15u : my_xcd()), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (4: a measuring switch — helpers nobody picks)
			const long long t0 = wall_clock64();
			int go = -1;
			for (;;) {
				const unsigned int v = __hip_atomic_load(w + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				if ((v >> 1) == a.dstamp) { go = (int) (v & 1u); break; }
				if (wall_clock64() - t0 > 200000000LL) break;
				__builtin_amdgcn_s_sleep(8);
			}
			if (go < 0) { atomicOr(a.flags, PHD_FLAG_ORDER_TIMEOUT); go = 0; }   // (cannot happen with workgroups handed out in order; the step is dropped)
			s_go[0] = go;
		}
		__syncthreads();
		const int go = s_go[0];
		__syncthreads();
		if (!go) return;
		// (the helper's sums are the longer of the two paths behind the hand-over: its waves go ahead of the main's where both sit on one
		// SIMD — 256 particles 0.0862 -> 0.0855 ms, profiles/r05_chain_helpers_prio.txt)
		__builtin_amdgcn_s_setprio(PHD_HELPER_PRIO);
		// every wave: what the main wrote in front of its word is in the L2 both share; this CU's L1 and the scalar cache may hold older lines
		__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
		asm volatile("s_dcache_inv\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
#ifdef PHD_STAMPS   // (slot 14: ticks from the main's hand-over to this point; slot 15: the helper's density sums, hand-over to end)
		const long long tw_ = wall_clock64();
		const bool fin_ = alpha_density_body(prm, a, smem, p, true, true, pre_pcount);
		if (threadIdx.x == 0 && a.stamps && a.stamp_kernel == 5) {
			const double t0_ = a.stamps[(size_t) p * 16 + 13];
			a.stamps[(size_t) p * 16 + 14] = (double) tw_ - t0_;
			a.stamps[(size_t) p * 16 + 15] = (double) wall_clock64() - t0_;
		}
		if (!fin_) return;
#else
		if (!alpha_density_body(prm, a, smem, p, true, true, pre_pcount)) return;
#endif
	}
	else {
	PHD_STAMP_DECL;
	PHD_STAMP(0);
	sweep_body<ZB, HALF, DEPTH>(prm, a, smem);
	__syncthreads();   // (workgroup scope: the global writes of the step before are visible to this workgroup's loads)
	PHD_STAMP(1);
	emit_finish_body<false, true, DEPTH>(prm, a, smem);
	__syncthreads();
	PHD_STAMP(2);
	prune_merge_body(prm, a, cutcap, smem);
	if (with_alpha) {
		__shared__ int s_hgo;
		if (threadIdx.x == 0) s_hgo = 0;
		__syncthreads();
		PHD_STAMP(3);
		alpha_assoc_body<ZB, false, false, 1, DEPTH>(prm, a, cutcap, smem, nullptr, a.dsplit ? &s_hgo : nullptr);
		__syncthreads();
		PHD_STAMP(4);
		// (every wave takes the flag into a register before thread 0 may reuse the word for alpha_meet's answer: without the
		// barrier a late wave could read that answer instead and take the other branch alone)
		const int hgo = s_hgo;
		__syncthreads();
		if (!hgo) alpha_density_body(prm, a, smem);
		else {
			// (the helper has the sums: this workgroup's number is the set log-likelihood it has just written)
			if (threadIdx.x == 0) {
				const int p = a.p0 + (int) blockIdx.x;
#ifdef PHD_STAMPS   // (slot 11: the association behind the hand-over, ticks)
				if (a.stamps && a.stamp_kernel == 5) a.stamps[(size_t) p * 16 + 11] = (double) wall_clock64() - a.stamps[(size_t) p * 16 + 13];
#endif
				const double sl = a.setll[p];
				__hip_atomic_store(a.setll + p, sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				s_hgo = alpha_meet(a, p, false, sl) ? 1 : 0;
			}
			__syncthreads();
			if (!s_hgo) return;
		}
		PHD_STAMP(5);
	}
	PHD_STAMP_FLUSH(5, 6);   // (diagnostic build, PHD_STAMP_KERNEL=5: the bodies' shares of the chain)
	}
}

// Test surface (phd_stage_map, PHD_STAGE_CORRECTED): the emitted list carries no mean / covariance for the misdetection
// copies (k_sweep writes their weight and index only); this fills them in from the predicted components.
__global__ __launch_bounds__(256) void k_expand_emit(const DevParams prm, const StepBufs a)
{
	const int p = a.p0 + blockIdx.x, tid = threadIdx.x;
	const MixView vin = bank_view(a, SEL_IN);
	const int n = vin.count[p], np = n + a.born_count[p], ne = a.emit_count[p];
	const size_t eb = (size_t) p * a.ecap;
	for (int e = tid; e < ne; e += 256) {
		const int cidx = a.emit_idx[eb + e];
		if (cidx < np) {
			double w, m[3], P[6];
			load_predicted(prm, a, vin, p, n, cidx, w, m, P);
			store_comp(a.emit_rec + (eb + e) * MIX_REC, a.emit_w[eb + e], m, P);
		}
	}
}

// The mixtures of the current state gathered into its own bank: particle i <- (INMIX, inslot[i]) written to (IN, i),
// after which INMIX = IN and the slots are the identity. Run before anything that addresses mixtures by particle
// number in bulk (uploads and downloads of whole states, single-map writes, the sharded step's migration).
// (the role INMIX = IN is written by the host once the launch has drained: a workgroup that did it here would redirect the
// reads of the workgroups that start after it)
__global__ __launch_bounds__(256) void k_materialise(const StepBufs a, int* inslot)
{
	const int i = blockIdx.x, tid = threadIdx.x;
	const MixView from = bank_view(a, SEL_IN);
	const Bank bi = bank_of(a, SEL_IN);
	const int n = bi.count[i];
	const size_t db = (size_t) i * a.cap, fb = in_base(a, i);
	copy_comps(bi.mix + db * MIX_REC, from.rec + fb * MIX_REC, n, tid, 256);
	__syncthreads();
	if (tid == 0) inslot[i] = i;   // only this workgroup reads inslot[i]
}

// Particle motion: TrackVehicle.UpdateNoisy (TrackVehicle.cs:89-102) = Pose3D.AddOdometry
// (Pose3D.cs:314-333) of the odometry reading, then of the particle's own noise vector (drawn by the host).
struct Quat4 { double w, x, y, z; };

__device__ __forceinline__ Quat4 quat_mul(const Quat4& a, const Quat4& b)   // Quaternion.cs:295-301
{
	return Quat4{a.w * b.w - (a.x * b.x + a.y * b.y + a.z * b.z),
	             a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
	             a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
	             a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}

__device__ inline void add_odometry(double s[7], const double* d)
{
	const Quat4 q{s[3], s[4], s[5], s[6]};
	const double l0 = 0.5 * d[3], l1 = 0.5 * d[4], l2 = 0.5 * d[5];   // FromLinear, Quaternion.cs:145-149
	const double phi = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
	Quat4 dq{1, 0, 0, 0};                                              // Exp, :185-196
	if (!(phi < 1e-12)) {
		const double sn = sin(phi);
		dq = Quat4{cos(phi), sn * (l0 / phi), sn * (l1 / phi), sn * (l2 / phi)};
	}
	const Quat4 nq = quat_mul(q, dq);
	Quat4 mid{1, 0, 0, 0};                                             // Sqrt, :225-235
	if (!(fabs(dq.w - -1.0) < 1e-8)) {
		const double rw = sqrt(0.5 * (1 + dq.w)), alpha = 1 / (2 * rw);
		mid = Quat4{rw, alpha * dq.x, alpha * dq.y, alpha * dq.z};
	}
	const Quat4 mr = quat_mul(q, mid);
	const Quat4 dl = quat_mul(quat_mul(mr, Quat4{0, d[0], d[1], d[2]}), Quat4{mr.w, -mr.x, -mr.y, -mr.z});
	const double alpha = 1 / sqrt(nq.w * nq.w + nq.x * nq.x + nq.y * nq.y + nq.z * nq.z);   // Normalize, :240-245
	s[0] += dl.x; s[1] += dl.y; s[2] += dl.z;
	s[3] = alpha * nq.w; s[4] = alpha * nq.x; s[5] = alpha * nq.y; s[6] = alpha * nq.z;
}

// (the bank holding the current poses is resolved here, on the device: correct right behind an asynchronous step)
__global__ __launch_bounds__(256) void k_motion(const StepBufs a, int P, const double* odometry, const double* noise, int use_noise)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= P) return;
	double* poses = bank_of(a, SEL_IN).poses;
	double s[7], d[6];
#pragma unroll
	for (int t = 0; t < 7; t++) s[t] = poses[(size_t) i * 7 + t];
#pragma unroll
	for (int t = 0; t < 6; t++) d[t] = odometry[t];
	add_odometry(s, d);
	if (use_noise) {
#pragma unroll
		for (int t = 0; t < 6; t++) d[t] = noise[(size_t) i * 6 + t];
		add_odometry(s, d);
	}
#pragma unroll
	for (int t = 0; t < 7; t++) poses[(size_t) i * 7 + t] = s[t];
}

// phd_set_poses / phd_set_weights: staged values into the small arrays of the current state (the IN bank, whichever
// it is by now). One thread per double.
__global__ __launch_bounds__(256) void k_store_small(const StepBufs a, const double* poses, const double* weights, int P)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	const Bank bi = bank_of(a, SEL_IN);
	if (poses && i < P * 7) bi.poses[i] = poses[i];
	if (weights && i < P) bi.weights[i] = weights[i];
}

// replicate particle 0 of the IN bank over `P` particles of the OUT bank (PHDNavigator.reset, :256-263)
__global__ __launch_bounds__(256) void k_replicate(const StepBufs a, double weight)
{
	const int i = blockIdx.x, tid = threadIdx.x;
	const MixView from = bank_view(a, SEL_IN), dst = bank_view(a, SEL_OUT);
	const int n = from.count[0];
	const size_t db = (size_t) i * a.cap, fb = in_base(a, 0);
	copy_comps(dst.rec + db * MIX_REC, from.rec + fb * MIX_REC, n, tid, 256);
	const Bank bi = bank_of(a, SEL_IN);
	const Bank bo = bank_of(a, SEL_OUT);
	if (tid == 0) {
		dst.count[i]  = n;
		bo.weights[i] = weight;
	}
	if (tid < 7) bo.poses[(size_t) i * 7 + tid] = bi.poses[tid];
}

// phd_test_detection_probability: detection_probability_m — the function the step's three call sites evaluate — on n
// pixel-range points, with the handle's parameters and current depth map
__global__ __launch_bounds__(256) void k_test_detection_probability(const DevParams prm, const double* __restrict__ z3, int n, double* __restrict__ out)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const double z[3] = {z3[(size_t) i * 3], z3[(size_t) i * 3 + 1], z3[(size_t) i * 3 + 2]};
	out[i] = prm.depth ? detection_probability_m<true>(prm, z, depth_at(prm, z)) : detection_probability_m(prm, z);
}
#endif   // PHD_ONLY_EP
