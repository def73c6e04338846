// phdhip.hip — host side of libphdhip.so: the C-ABI of include/phdhip.h over the kernels of
// phd_kernels.h. Built for gfx950 only:  hipcc --offload-arch=gfx950 -O3 -shared -fPIC
//
// There is no CPU implementation behind this ABI: without a HIP device phd_create fails with
// PHD_ERR_NO_DEVICE and every other entry point needs a handle.
#include "../../include/phdhip.h"
#include "phd_kernels.h"
#include "phd_history.h"
#include "phd_maplog.h"
#include "phd_maperror.h"
#include "phd_poseerror.h"
#include "phd_ascent.h"
#include "phd_ascent_multi.h"
#include "phd_guesses.h"
#include "phd_hold.h"
#include "phd_primitives_test.h"   // (last of the headers: k_test_primitive is the last kernel that is no template; the instantiations follow it)
#include "../host/Ospa.hpp"   // MapErrorAlignment: the alignment of phd_map_error is the host metric's, computed by the same function

#include <algorithm>
#include <cstdint>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <utility>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <functional>
#include <vector>

#define DSPLIT_ROWS 1024     // particles the helpers' words are allocated for (k_particle_chain with helper workgroups)

namespace {

thread_local std::string g_create_error;

struct Timer {          // one record per kernel launch since the last phd_timing_reset
	const char* name;
	hipEvent_t  t0, t1;
	int         t0_from;   // >= 0: the launch starts where record t0_from ended (back-to-back on one stream: one event, not two)
};

// What a handle allocates, released when its owner goes (move-only); the owner converts to the raw pointer wherever one is
// read. K says how one kind of resource is made and released. The device of the handle must be current when an owner goes.
struct DevMem  { static hipError_t make(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); } static void drop(void* p) { hipFree(p); } };
struct PinMem  { static hipError_t make(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); } static void drop(void* p) { hipHostFree(p); } };
struct EventK  { static void drop(hipEvent_t e) { hipEventDestroy(e); } };
struct StreamK { static void drop(hipStream_t s) { hipStreamDestroy(s); } };

template <class T, class K>
class Owned {
	T* p_ = nullptr;
public:
	using element = T;
	Owned() = default;
	Owned(const Owned&) = delete;
	Owned& operator=(const Owned&) = delete;
	Owned(Owned&& o) noexcept : p_(o.release()) {}
	Owned& operator=(Owned&& o) noexcept { if (this != &o) reset(o.release()); return *this; }
	~Owned() { reset(); }
	operator T*() const { return p_; }
	void reset(T* p = nullptr) { if (p_) K::drop(p_); p_ = p; }
	T* release() { T* p = p_; p_ = nullptr; return p; }   // (gives the resource up without releasing it)
	T** put() { reset(); return &p_; }                   // for the runtime's creating calls with an out-parameter
	hipError_t alloc(size_t count, unsigned flags = 0) { return K::make((void**) put(), count * sizeof(T), flags); }   // `count` elements; what it held goes first
};
template <class T> using DevBuf = Owned<T, DevMem>;
template <class T> using PinBuf = Owned<T, PinMem>;
using Event  = Owned<ihipEvent_t, EventK>;
using Stream = Owned<ihipStream_t, StreamK>;

}  // namespace

struct MultiState;   // phd_create_multi: the shards of a multi-device handle (phd_multi.inc)

struct phd_navigator {
	MultiState* multi = nullptr;       // non-NULL: this handle only dispatches to its shards
	phd_params  prm;
	DevParams   dp;
	int         device = 0;
	hipStream_t stream = nullptr;      // the stream every kernel of this handle is launched on
	Stream      own_stream;            // created by phd_create; `stream` unless the host lent its own (a lent stream is not the handle's to destroy)
	static const int MAXSPLIT = 4;
	int         nsplit = 0;            // sub-ranges a step's per-particle kernels are split into (0: chosen from the particle count)
	int         dsplit_max = 256;      // ... and up to this many, with a helper workgroup per particle for the densities of WeightAlpha (two workgroups per
	                                   // particle: 2 P workgroups fit the chip's 512 slots of that kernel at once; env PHD_DSPLIT_MAX, 0: never)
	int         dsplit_late = 0;       // env PHD_DSPLIT_LATE (tests and measurements; StepBufs::dsplit = 1 + this): 1 the helpers report 0.5 ms late, 2 they leave at once,
	                                   // 3 they report and wait but are never picked — in all three every main workgroup keeps its density sums
	unsigned int dseq = 0;             // launches of the chain with helpers so far (StepBufs::dstamp)
	DevBuf<unsigned int> d_dsync;      // the helpers' words (StepBufs); DSPLIT_ROWS particles
	int         chain_max = 512;       // up to this many particles a step's per-particle kernels run as one launch (k_particle_chain; env PHD_CHAIN_MAX)
	bool        chain_ok[3] = {false, false, false};   // ... where the bodies' LDS arrays fit one workgroup (per measurement-block count 1, 2, 4)
	Stream      aux[MAXSPLIT - 1];     // streams of the sub-ranges after the first
	int         fuse_ep = -1;          // k_emit_finish and k_prune_merge as one launch (k_emit_prune): -1 = for frames of up to 64 measurements (measured on
	                                   // two streams: config B 0.677 -> 0.667 ms survey, 0.634 -> 0.615 steady; config S, 128 measurements, 3.67 -> 3.85:
	                                   // its Kalman path is long and pays for the 128 registers); environment PHD_FUSE_EP = 0 / 1 forces
	DevBuf<double> d_ratio;            // [Pcap] StepBufs::ratio
	Event       ev_fork, ev_join[MAXSPLIT - 1];
	// Two sub-ranges, steps posted back to back (phd_step_async after phd_step_async): the end of the step runs on the stream
	// whose chain finishes LAST and no fork precedes the next step ("the step boundary"; env PHD_PIPELINE=0: a fork
	// before and a join behind every step, as for every other caller)
	int         pipeline = 1;
	bool        pipe_ok = false;       // nothing was enqueued on `stream` since the last such step: the aux stream is ordered behind all of it
	int         lagger = 1;            // which of the two streams (0 `stream`, 1 aux[0]) finishes the coming step last
	Event       ev_res;                // k_normalise_resample is through (recorded on the stream that ran it)
	bool sel_host_valid = false;       // h_sel mirrors the device-side bank roles without a round trip
	int Pcap = 0, cap = 0, Mcap = 0, ecap = 0, Jcap = 0, cutcap = 0;
	int P = 0, M = 0;
	bool frozen = false;
	bool all_pairs = false;            // phd_set_all_pairs: the benchmark mode of SURVEY §8d

	Bank   bank[3];              // (plain pointers: kernels take it by value; its arrays are owned beside it)
	DevBuf<double> bank_mix[3], bank_poses[3], bank_weights[3]; DevBuf<int> bank_count[3];
	DevBuf<int> d_sel;           // [2][SEL_STRIDE]: roles for the current / next step (+ where the last result is)
	DevBuf<int> d_mslot;         // [Pcap] sharded step: slot of every particle's mixture in the OUT bank
	const int* d_res_slots = nullptr;   // slots of the last step's result in RESMIX (frozen mode getters)
	DevBuf<int> d_inslot;        // [Pcap] slot of every particle's mixture in the INMIX bank (identity unless the last step resampled)
	int    parity = 0;
	int    h_sel[SEL_STRIDE] = {0, 1, 2, 0, 0, 0, 0, 0};

	DevBuf<double> d_z;
	DevBuf<double> d_emit_w; DevBuf<int> d_emit_idx; DevBuf<double> d_emit_rec; DevBuf<int> d_emit_count;
	DevBuf<int>    d_born_count, d_born_k; DevBuf<double> d_born_mean;
	DevBuf<double> d_alpha, d_setll;
	int*    d_flags = nullptr; DevBuf<int> d_src; int* d_info = nullptr;   // (d_info, d_flags: words of d_sel's block)
	DevBuf<MurtyNodes> d_murty;
	DevBuf<char> d_bigws; unsigned long long bigws_bytes = 0; DevBuf<unsigned long long> d_bigws_used;   // association slab (clusters beyond 64 rows)
	DevBuf<double> d_jscratch;
	int cmcap = 0;
	DevBuf<int> d_cand_count; DevBuf<double> d_denom;
	DevBuf<int> d_cand; int candcap = 0;
	DevBuf<double> d_alm; DevBuf<int> d_aJ; DevBuf<double> d_account;
	DevBuf<double> d_stamps;
	DevBuf<double> d_srec;
	DevBuf<double> d_outw;        // [Pcap][cap] the pruned weights as a plane (StepBufs::outw)
	DevBuf<double> d_wcopy; DevBuf<int> d_cover;   // k_prune_merge -> k_alpha_density (see StepBufs)
	DevBuf<double> d_motion;      // odometry[6] + noise[P][6] of phd_update_motion
	DevBuf<double> d_hold; DevBuf<int> d_hold_count;   // phd_step_hold_async: the held slot's records [cap][10] and their count (phd_hold.h), made on first use
	DevBuf<double> d_quasi;       // phd_quasi_set_loglik: poses[Pcap][7], landmarks[Jcap][3], z[256][3], out[Pcap]
	PinBuf<int>    h_status;      // pinned mirror of [d_sel (two parities) | d_info | d_flags], one block on the device
	PinBuf<double> h_quasi;       // ... its pinned mirror on the host (+ one word for the flags): one stream wait per call, no pageable copies
	DevBuf<double> d_ascent;      // phd_quasi_ascent: the inputs, the per-estimate state and the results of one call (ascent_layout), made on first use
	PinBuf<double> h_ascent;      // ... the pinned mirror of what is copied in and out, and the word the host reads between rounds
	DevBuf<double> d_amulti;      // phd_quasi_ascent_multi / phd_quasi_set_loglik_multi: the same for a call over many problems (multi_layout); grows to the largest call
	PinBuf<double> h_amulti;
	size_t amulti_cap = 0;        // doubles either holds
	DevBuf<double> d_guess;       // phd_quasi_guesses_multi: the problems of a call, its tile words and its flag word and slab counter (guess_layout); grows to the largest call
	PinBuf<double> h_guess;
	size_t guess_cap = 0;
	DevBuf<double> d_gout;        // ... and what it makes per guess (guess_out_layout), sized once the total is known
	PinBuf<double> h_gout;
	size_t gout_cap = 0;
	DevBuf<double> d_gw; int gwcap = 0;              // gathered weights of all ranks (+ their status words behind them: flagslot)
	DevBuf<double> d_stage;                          // device staging of phd_set_poses / phd_set_weights (stored into the IN bank by k_store_small)
	// pinned host staging of the per-frame inputs (poses, weights, odometry + noise, measurements): the caller's buffers are
	// copied here and are free when the call returns; the copy to the device is asynchronous. Two buffers, each guarded by
	// an event recorded behind the copy that reads it.
	PinBuf<double> h_stage[2]; Event ev_stage[2]; bool stage_used[2] = {false, false};
	int stage_i = 0; size_t stagecap = 0;
	// the depth map of phd_set_depth_map (KinectMeasurer): the device copy dp.depth points at (depthcap floats, grown on demand) and
	// its own pair of pinned staging slots, guarded like h_stage (hdepthcap floats each)
	DevBuf<float> d_depth; size_t depthcap = 0;
	PinBuf<float> h_depth[2]; Event ev_depth[2]; bool depth_used[2] = {false, false};
	int depth_i = 0; size_t hdepthcap = 0;
	int nr_static_lds = 0;                           // static LDS of k_normalise_resample
	// the step over a grid of workgroups (k_nr_*, phd_resample.h) for weight vectors of nr_grid_min .. 65 536 entries (environment
	// PHD_NR_GRID_MIN; 0: never): its scratch, made on first use
	int nr_grid_min = NR_GRID_MIN; int nrcap = 0; DevBuf<double> d_nrd; DevBuf<int> d_nri;
	// sharded step (one rank of a multi-GPU particle set: a process of its own, or a shard of a phd_create_multi handle)
	DevBuf<double>  d_lw;                            // [Pcap] local weights, exported for the host's all-gather (per-rank host)
	DevBuf<double*> d_dst_tab; int ndst = 1;         // device table: where k_push_weights stores the local weights (own d_lw | every shard's d_gw)
	int      push_first = 0, push_flagslot = -1;     // ... at which offset, and where the status word goes (-1: nowhere)
	DevBuf<double*> d_recv_tab;                      // device table: the receive buffer of every shard / rank (filled by phd_create_multi, phd_migration_set_peers / _ipc_open)
	bool peers_set = false;                          // ... it is filled: migrating particles can be pushed
	bool gw_shared = false;                          // other shards hold the address of d_gw (multi-device handle): it cannot grow
	const double* d_gflags = nullptr;                // the gathered status words (multi-device handle)
	DevBuf<double> d_send, d_recv; DevBuf<int> d_plan; int sendrecs = 0, recvrecs = 0;
	MigPlan plan = {nullptr, nullptr, nullptr, nullptr, nullptr, 0};   // device-resident migration plan (k_plan_migration); plain pointers as the banks, owned by:
	DevBuf<int> plan_code, plan_fslot, plan_sendlist, plan_counts; DevBuf<long long> plan_senddst;
	// the plan over a grid of workgroups (k_plan_count / k_plan_lists) for global vectors of plan_grid_min .. 65 536 slots whose
	// ranks hold a multiple of 64 particles (environment PHD_PLAN_GRID_MIN; 0: never): its accumulators (two sets, alternating)
	int plan_grid_min = PLAN_GRID_MIN; DevBuf<int> d_plang; int plan_par = 0;
	PinBuf<int> h_counts; int plan_seq = 0;          // pinned + mapped: the plan's counts as the kernel writes them, and the word the host polls
	bool plan_waiting = false;                       // a plan kernel with host counts is in flight
	int world = 1, rank = 0;                         // of the last global step
	int nsend = 0, nrecv = 0, last_world_particles = 1;
	bool sharded_used = false;
	bool sharded_ready = false;                      // every buffer of ensure_sharded is there (set behind the last allocation)
	bool recv_finegrained = false;                   // d_recv is fine-grained device memory (coherent for the peers that store into it)
	int  landing_flags = 0;                          // phd_migration_set_landing: 1 = push posts step-stamped flags into the peers' receive buffers, unpack waits for them
	unsigned long long landing_seq = 0;              // number of the last device-path global step (the flags' stamp)
	long long landing_ticks = 1000000000LL;          // bound of the wait for a flag, in ticks of the 100 MHz counter: 10 s (environment PHD_LANDING_TIMEOUT_MS)
	DevBuf<double> d_graw; int grawcap = 0;          // per-rank host: the all-gather's landing buffer, [world][P + 1] (weights | status word)
	std::vector<void*> ipc_opened;                   // peers' receive buffers opened with hipIpcOpenMemHandle (closed in phd_destroy)
	bool plan_on_device = false;                     // the last global step left its plan on the device only (phd_step_global_device_async)
	// the trajectory log (phd_history_enable; phd_history.h): hist_cap entries of Pcap particles, hist_len of them written; hist_pp:
	// which copy of pend is current (flipped by every launch that writes the other one); the times stay on the host
	int hist_cap = 0, hist_len = 0, hist_pp = 0;
	DevBuf<double> d_hpose; DevBuf<int> d_hparent, d_hdirty, d_hpend;   // d_hpend: [2][Pcap] | the two dirty words
	std::vector<double> h_htimes;
	// phd_trajectories: the requested particles and the paths on the device, their pinned mirrors on the host (grown on demand)
	DevBuf<int> d_tq, d_tslot; DevBuf<double> d_tpose; PinBuf<int> h_tq, h_tslot; PinBuf<double> h_tpose; size_t tqcap = 0, tcap = 0;
	int* hpend(int which) { return d_hpend + (size_t) which * Pcap; }
	int* hpdirty(int which) { return d_hpend + 2 * (size_t) Pcap + which; }
	// the map log (phd_map_history_enable; phd_maplog.h): mlog_cap entries over mlog_comps component records, mlog_len of them
	// appended; mlog_pp: which copy of the bump word is current; the times stay on the host
	int mlog_cap = 0, mlog_len = 0, mlog_pp = 0; long long mlog_comps = 0;
	DevBuf<double> d_mlrec; DevBuf<MapLogEntry> d_mlentry; DevBuf<long long> d_mlbump;
	std::vector<double> h_mltimes, h_mlrec, h_mlpose, h_mlw, h_mlm, h_mlc;
	std::vector<MapLogEntry> h_mlentry; std::vector<int32_t> h_mlbest, h_mlcount; std::vector<int64_t> h_mloff;
	// phd_map_error (phd_maperror.h): the truth set and the alignment of every entry on the device, the results ([3][mecap] doubles:
	// ospa | cardinality | spatial; [mecap] sizes and the flag word behind them) and their host mirrors; grown on demand
	DevBuf<double> d_metruth, d_mealign, d_meout; DevBuf<int> d_mesize; int mecap = 0;
	std::vector<double> h_mealign, h_meout; std::vector<int32_t> h_mesize;
	// phd_pose_error (phd_poseerror.h). Per trajectory-log entry, written by phd_history_append: the map log's length at that
	// moment — what slots == NULL resolves the estimates from. They name entries of today's map log if it has been on and not
	// restarted since the trajectory log's first entry: mlog_epoch counts its restarts (every switch on or off is one), and
	// hist_mepoch is that count when the first entry was made, -1 if the map log was off then. Epochs only grow, so the first
	// entry's speaks for all of them, and within one epoch the map log only grows, so no mark lies behind its end.
	// The truth rows, the slots (or those marks) and the Timed start indices on the device, the results ([4][pecap] doubles:
	// location | rotation | odometry location | odometry rotation) and the host mirrors handed out; grown on demand
	int mlog_epoch = 0, hist_mepoch = -1;
	std::vector<int> h_hmark;
	DevBuf<double> d_petruth, d_peout; DevBuf<int> d_pesel, d_pestart; int pecap = 0;
	std::vector<double> h_peout, h_petimes, h_peodotimes; std::vector<int> h_pesel, h_pestart;
	// host mirrors handed out by the getters
	std::vector<double> h_weights, h_poses, h_mw, h_mm, h_mc, h_alpha, h_setll, h_tmp;
	std::vector<int32_t> h_src;
	int  h_info[2] = {0, 0};
	int  h_flags = 0;
	bool stage_valid = false;

	std::vector<Timer>       timers;    // event pool; [0, ntimers) are live records
	size_t                   ntimers = 0;
	bool                     timing = true;
	int                      timing_period = 1;   // launches are timed on every timing_period-th step
	long long                timing_step = 0;
	bool                     timing_now = true;
	std::vector<const char*> tnames;
	std::vector<double>      tms;
	std::vector<int>         tcounts;
	std::string err;

	int fail(int code, const std::string& what)
	{
		err = what;
		return code;
	}
};

namespace {

#define HC(call)                                                                                    \
	do {                                                                                            \
		hipError_t e_ = (call);                                                                     \
		if (e_ != hipSuccess) {                                                                     \
			return nav->fail(PHD_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_));    \
		}                                                                                           \
	} while (0)

void inv3_host(const double* a, double* inv, double* det)
{
	double c00 = a[4] * a[8] - a[5] * a[7];
	double c01 = a[3] * a[8] - a[5] * a[6];
	double c02 = a[3] * a[7] - a[4] * a[6];
	double d   = a[0] * c00 - a[1] * c01 + a[2] * c02;
	double id  = 1.0 / d;
	inv[0] = c00 * id;
	inv[1] = (a[2] * a[7] - a[1] * a[8]) * id;
	inv[2] = (a[1] * a[5] - a[2] * a[4]) * id;
	inv[3] = (a[5] * a[6] - a[3] * a[8]) * id;
	inv[4] = (a[0] * a[8] - a[2] * a[6]) * id;
	inv[5] = (a[2] * a[3] - a[0] * a[5]) * id;
	inv[6] = c02 * id;
	inv[7] = (a[1] * a[6] - a[0] * a[7]) * id;
	inv[8] = (a[0] * a[4] - a[1] * a[3]) * id;
	*det = d;
}

DevParams make_dev_params(const phd_params& p)
{
	DevParams d;
	d.focal  = p.measurer[0];
	d.rmin   = (double) (float) p.measurer[1];   // AForge.Range is float32 (PRM3DMeasurer.cs:65,110)
	d.rmax   = (double) (float) p.measurer[2];
	d.left   = (double) (int) p.measurer[3];     // XNA Rectangle is int (PRM3DMeasurer.cs:111)
	d.top    = (double) (int) p.measurer[4];
	d.right  = (double) ((int) p.measurer[3] + (int) p.measurer[5]);
	d.bottom = (double) ((int) p.measurer[4] + (int) p.measurer[6]);
	for (int i = 0; i < 3; i++) d.ramp[i] = p.visibility_ramp[i];
	for (int i = 0; i < 9; i++) d.R[i] = p.R[i];
	d.linear2d  = p.model == PHD_MODEL_LINEAR2D ? 1 : 0;
	d.lin_range = p.measurer[0];
	if (d.linear2d) {   // R is 2 x 2 row-major in the first four entries: pad it with a unit third coordinate (DevParams)
		const double r2[4] = {p.R[0], p.R[1], p.R[2], p.R[3]};
		const double r3[9] = {r2[0], r2[1], 0, r2[2], r2[3], 0, 0, 0, 1};
		for (int i = 0; i < 9; i++) d.R[i] = r3[i];
		d.ramp[2] = 1.0;
	}
	double det;
	inv3_host(d.R, d.Rinv, &det);
	d.logRmult = std::log(std::pow(2 * 3.14159265358979323846, -1.0) / std::sqrt(std::fabs(det)));
	d.pd       = p.pd;
	d.kappa    = p.clutter_density;
	d.logkappa = std::log(p.clutter_density);
	const double* B = p.birth_covariance;
	d.birthP[0] = B[0]; d.birthP[1] = B[1]; d.birthP[2] = B[2]; d.birthP[3] = B[4]; d.birthP[4] = B[5]; d.birthP[5] = B[8];
	d.birthw     = p.birth_weight;
	d.minw       = p.min_weight;
	d.expl_thr   = p.exploration_threshold;
	// Map.Near / Map.Evaluate(x, radius): Accord's KDTree compares its distance with the radius; with the
	// squared-Euclidean metric that is |x-m|^2 <= radius, with the Euclidean one |x-m| <= radius
	const double rc = p.density_distance_threshold, re = 3 * p.density_distance_threshold;
	d.g2_correct = (p.gate_metric == PHD_GATE_DISABLED) ? INFINITY : (p.gate_metric == PHD_GATE_SQUARED_EUCLIDEAN ? rc : rc * rc);
	d.g2_explore = (p.gate_metric == PHD_GATE_DISABLED) ? INFINITY : (p.gate_metric == PHD_GATE_SQUARED_EUCLIDEAN ? re : re * re);
	d.merge_thr2 = p.merge_threshold * p.merge_threshold;
	d.g2_assoc = 25.0;
	while (std::sqrt(std::nextafter(d.g2_assoc, 0.0)) >= 5.0) d.g2_assoc = std::nextafter(d.g2_assoc, 0.0);
	d.g2_quasi = 144.0;
	while (std::sqrt(std::nextafter(d.g2_quasi, 0.0)) >= 12.0) d.g2_quasi = std::nextafter(d.g2_quasi, 0.0);
	d.min_eff    = p.min_effective_particle;
	double floor = p.min_weight * p.clutter_density;
	d.emit_log_floor = (floor > 0) ? std::log(floor) : -INFINITY;
	d.gate_metric = p.gate_metric;
	d.maxq        = p.max_quantity;
	d.depth = nullptr; d.depth_w = 0; d.depth_h = 0; d.depth_hx = 0; d.depth_hy = 0;   // no depth map: phd_set_depth_map
	return d;
}

StepBufs make_bufs(phd_navigator* nav)
{
	StepBufs b;
	b.P = nav->P; b.p0 = 0; b.qposes = nullptr; b.qlm = nullptr; b.qJ = 0; b.cap = nav->cap; b.M = nav->M; b.Mcap = nav->Mcap; b.ecap = nav->ecap; b.Jcap = nav->Jcap;
	for (int i = 0; i < 3; i++) b.bank[i] = nav->bank[i];
	b.sel = nav->d_sel + nav->parity * SEL_STRIDE;
	b.inslot = nav->d_inslot;
	b.z = nav->d_z;
	b.emit_w = nav->d_emit_w; b.emit_idx = nav->d_emit_idx; b.emit_rec = nav->d_emit_rec; b.emit_count = nav->d_emit_count;
	b.born_count = nav->d_born_count; b.born_k = nav->d_born_k; b.born_mean = nav->d_born_mean;
	b.alpha = nav->d_alpha; b.setll = nav->d_setll; b.flags = nav->d_flags; b.murty = nav->d_murty; b.jscratch = nav->d_jscratch;
	b.bigws = nav->d_bigws; b.bigws_bytes = nav->bigws_bytes; b.bigws_used = nav->d_bigws_used;
	b.cand_count = nav->d_cand_count; b.denom = nav->d_denom;
	b.cand = nav->d_cand; b.candcap = nav->candcap;
	b.dsplit = 0; b.dstamp = 0; b.dsync = nav->d_dsync;
	b.alm = nav->d_alm; b.aJ = nav->d_aJ; b.account = nav->d_account; b.srec = nav->d_srec; b.outw = nav->d_outw; b.wcopy = nav->d_wcopy; b.cover = nav->d_cover; b.stamps = nav->d_stamps; b.ratio = nav->d_ratio; b.all_pairs = nav->all_pairs ? 1 : 0; b.emit_all = 0; b.stamp_kernel = getenv("PHD_STAMP_KERNEL") ? atoi(getenv("PHD_STAMP_KERNEL")) : 2;
	return b;
}

// Every entry point that may enqueue work on the handle's stream comes through here (phd_step_async alone does not): whatever
// it enqueues, the aux stream is not ordered behind it until the next step forks again.
static inline void enter(phd_navigator* nav)
{
	hipSetDevice(nav->device);
	nav->pipe_ok = false;
}

// Non-finite numbers do not cross the ABI (include/phdhip.h, "Non-finite input"): the reference lets a NaN term poison a
// whole weight sum (PHDNavigator.cs:886-890) where the device's pair loops count a NaN exponent as 0 (exp_pair); with
// finite input the two never meet.
bool all_finite(const double* v, size_t n)
{
	if (!v) return true;
	unsigned long long bad = 0;
	for (size_t i = 0; i < n; i++) {
		unsigned long long b;
		std::memcpy(&b, v + i, 8);
		bad |= (unsigned long long) ((b & 0x7ff0000000000000ull) == 0x7ff0000000000000ull);
	}
	return bad == 0;
}
#define FINITE_OR_FAIL(nav, ptr, n, who) do { if (!all_finite((ptr), (size_t) (n))) return (nav)->fail(PHD_ERR_BAD_ARGUMENT, who ": non-finite input (NaN or infinity) is not accepted"); } while (0)

// A pinned staging buffer nobody reads any more (waits for the copy that last read it: normally long done).
double* stage_acquire(phd_navigator* nav)
{
	nav->stage_i ^= 1;
	const int i = nav->stage_i;
	if (nav->stage_used[i]) hipEventSynchronize(nav->ev_stage[i]);
	return nav->h_stage[i];
}

// ... the asynchronous copy out of it has been enqueued on the handle's stream
void stage_release(phd_navigator* nav)
{
	hipEventRecord(nav->ev_stage[nav->stage_i], nav->stream);
	nav->stage_used[nav->stage_i] = true;
}


// HIP events around every kernel launch, on the stream the kernel is launched on: the scope of a Timed is one record.
// `chained`: the launch follows the previous timed launch on the same stream with nothing in between, so that launch's end
// event is this one's start.
struct Timed {
	phd_navigator* nav;
	hipStream_t    st;
	Timed(phd_navigator* nav_, const char* name, hipStream_t st_, bool chained = false) : nav(nav_), st(st_)
	{
		if (!nav->timing || !nav->timing_now) return;
		if (nav->ntimers == nav->timers.size()) {
			if (nav->timers.size() >= 65536) { nav->timing = false; return; }
			Timer t;
			t.name = name;
			t.t0_from = -1;
			// (timing only, read after a stream synchronisation: no system-scope fence when they are recorded — the fence of a default event
			// writes the caches back in front of every timed launch and is part of what the step then costs)
			if (hipEventCreateWithFlags(&t.t0, hipEventDisableSystemFence) != hipSuccess || hipEventCreateWithFlags(&t.t1, hipEventDisableSystemFence) != hipSuccess) {
				(void) hipGetLastError();
				if (hipEventCreate(&t.t0) != hipSuccess || hipEventCreate(&t.t1) != hipSuccess) { nav->timing = false; return; }
			}
			nav->timers.push_back(t);
		}
		Timer& t = nav->timers[nav->ntimers];
		t.name = name;
		t.t0_from = (chained && nav->ntimers > 0) ? (int) nav->ntimers - 1 : -1;
		if (t.t0_from < 0) hipEventRecord(t.t0, st);
	}
	~Timed()
	{
		if (!nav->timing || !nav->timing_now || nav->ntimers >= nav->timers.size()) return;
		hipEventRecord(nav->timers[nav->ntimers].t1, st);
		nav->ntimers++;
	}
	Timed(const Timed&) = delete;
	Timed& operator=(const Timed&) = delete;
};

// one kernel launch as one record
template <class... KA, class... A>
void launch_timed(phd_navigator* nav, const char* name, hipStream_t st, bool chained, void (*kernel)(KA...), dim3 grid, dim3 block, size_t lds, const A&... args)
{
	Timed t(nav, name, st, chained);
	hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}

const char* T_SW = "k_sweep";
const char* T_EF = "k_emit_finish";
const char* T_PM = "k_prune_merge";
const char* T_EP = "k_emit_prune";
const char* T_WA = "k_alpha_assoc";
const char* T_WD = "k_alpha_density";
const char* T_NR = "k_normalise_resample";
const char* T_GR = "k_finish_sharded";
const char* T_PL = "k_plan_migration";
const char* T_PK = "k_pack_particles";
const char* T_PW = "k_push_weights";
const char* T_CH = "k_particle_chain";

// The per-particle kernels of a step are compiled per measurement-block count ZB (64 measurements a block), for up to 32
// measurements with the sweep that takes two components per visit (HALF, phd_sweep.h; one block only), and with the Kinect
// detection probability of a depth map (DEPTH, phd_device.h). One row per build: its kernels and the dynamic LDS each asks
// for at a handle's max_quantity. (k_quasi_setll / _grad have no HALF or DEPTH build: every row of a ZB names the same two.)
struct StepVariant {
	int  zb;
	bool half, depth;
	void (*chain)(DevParams, StepBufs, int, int);
	void (*sweep)(DevParams, StepBufs);
	void (*emit_prune)(DevParams, StepBufs, int);
	void (*emit_finish)(DevParams, StepBufs);
	void (*assoc)(DevParams, StepBufs, int);
	void (*quasi)(DevParams, StepBufs, int);
	void (*quasi_grad)(DevParams, StepBufs, int);
	void (*ascent)(DevParams, StepBufs, int, const int*, int);        // the same two bodies for phd_quasi_ascent: workgroups of stopped estimates return
	void (*ascent_grad)(DevParams, StepBufs, int, const int*, int);
	void (*multi)(DevParams, StepBufs, int, QuasiProblems, const int*, int);   // ... with the landmark and measurement set of the estimate's problem bound in (phd_ascent_multi.h)
	void (*multi_grad)(DevParams, StepBufs, int, QuasiProblems, const int*, int);
	int  (*chain_pool)(int);
	int zi() const { return zb >> 1; }   // index of ZB = 1, 2, 4 (phd_navigator::chain_ok)
	int chain_lds(int cutcap) const { return chain_pool(cutcap); }
	int assoc_lds(int cutcap) const { return alpha_lds(zb * 64, cutcap).bytes; }
	static int emit_prune_lds(int cutcap) { return std::max((int) prune_lds(cutcap).bytes, (int) (EMIT_LDS_DOUBLES * 8)); }
};

template <int ZB, bool HALF, bool DEPTH>
StepVariant make_variant()
{
	return {ZB, HALF, DEPTH, k_particle_chain<ZB, HALF, DEPTH>, k_sweep<ZB, HALF, DEPTH>, k_emit_prune<DEPTH>, k_emit_finish<DEPTH>, k_alpha_assoc<ZB, DEPTH>,
	        k_quasi_setll<ZB>, k_quasi_setll_grad<ZB>, k_ascent_setll<ZB>, k_ascent_setll_grad<ZB>, k_multi_setll<ZB>, k_multi_setll_grad<ZB>, chain_lds_bytes<ZB>};
}

const StepVariant step_variants[8] = {make_variant<1, false, false>(), make_variant<1, true, false>(), make_variant<2, false, false>(), make_variant<4, false, false>(),
                                      make_variant<1, false, true>(),  make_variant<1, true, true>(),  make_variant<2, false, true>(),  make_variant<4, false, true>()};

int zb_of(int M) { return M <= 64 ? 1 : (M <= 128 ? 2 : 4); }

// The build that serves a step of M measurements, with or without a depth map: the one statement of that rule.
const StepVariant& variant(int M, bool depth_set)
{
	const int zb = zb_of(M);
	const bool half = zb == 1 && M <= 32;
	for (const StepVariant& v : step_variants) {
		if (v.zb == zb && v.half == half && v.depth == depth_set) return v;
	}
	return step_variants[0];   // (not reached: the table holds every combination the rule yields)
}

// The per-particle kernels of a step. With nsplit > 1 the particle range is cut into sub-ranges whose kernel
// chains run on concurrent streams (forked from and joined back into the handle's stream), so that the
// latency-bound kernels of one sub-range overlap the arithmetic-bound kernels of another.
// `pipe` >= 0 (phd_step_async, two sub-ranges): no fork and no join here — the caller has ordered the streams and ends the step on
// the stream that finishes last, `pipe` (0 `stream`, 1 aux[0]); the other one's chain is enqueued first.
int launch_map(phd_navigator* nav, const StepBufs& b0, bool with_alpha, int pipe = -1)
{
	const StepVariant& v = variant(nav->M, nav->dp.depth != nullptr);
	const int P = nav->P, cutcap = nav->cutcap;
	// two half-ranges measured best at 2048 particles (1.10 -> 1.02 ms); below ~4 workgroups per CU and sub-range it does not pay
	const int want = nav->nsplit > 0 ? nav->nsplit : (P >= 1024 ? 2 : 1);
	const int S = std::max(1, std::min(std::min(want, (int) phd_navigator::MAXSPLIT), P));
	const size_t lp = (size_t) prune_lds(cutcap).bytes;   // (the dynamic LDS limits of the kernels were raised once, in phd_create)
	const dim3 block(256);
	const int wa = with_alpha ? 1 : 0;
	if (nav->chain_ok[v.zi()] && P <= nav->chain_max) {
		// a small particle set (up to two workgroups per CU): the whole per-particle chain as one launch
		// (a helper workgroup per particle for the densities when all 2 P workgroups can be on the chip together; the results are the
		// same bits whether a helper comes in time or not: k_particle_chain)
		StepBufs bc = b0;
		const bool helpers = with_alpha && nav->d_dsync && P <= nav->dsplit_max && P <= DSPLIT_ROWS;
		if (helpers) {
			if (++nav->dseq >= 0x07ffffffu) {   // (the numbers start again: no word of an earlier round may be taken for one of this round)
				nav->dseq = 1;
				HC(hipMemsetAsync(nav->d_dsync, 0, (size_t) std::min(nav->Pcap, (int) DSPLIT_ROWS) * 3 * 4, nav->stream));
			}
			bc.dsplit = nav->dsplit_late > 0 ? 1 + nav->dsplit_late : 1; bc.dstamp = nav->dseq;
		}
		launch_timed(nav, T_CH, nav->stream, false, v.chain, dim3(helpers ? 2 * P : P), block, (size_t) v.chain_lds(cutcap), nav->dp, bc, cutcap, wa);
		HC(hipGetLastError());
		return PHD_OK;
	}
	if (S > 1 && pipe < 0) {
		HC(hipEventRecord(nav->ev_fork, nav->stream));
		for (int s = 1; s < S; s++) HC(hipStreamWaitEvent(nav->aux[s - 1], nav->ev_fork, 0));
	}
	const size_t la = (size_t) v.assoc_lds(cutcap);
	for (int si = 0; si < S; si++) {
		const int s = (pipe >= 0 && S == 2) ? (si == 0 ? 1 - pipe : pipe) : si;
		StepBufs b = b0;
		b.p0 = (int) ((long long) P * s / S);
		const int n = (int) ((long long) P * (s + 1) / S) - b.p0;
		if (n <= 0) continue;
		hipStream_t st = s == 0 ? nav->stream : (hipStream_t) nav->aux[s - 1];
		const dim3 grid(n);
		launch_timed(nav, T_SW, st, false, v.sweep, grid, block, 0, nav->dp, b);
		if (nav->fuse_ep < 0 ? v.zb == 1 : nav->fuse_ep != 0) {
			launch_timed(nav, T_EP, st, true, v.emit_prune, grid, block, (size_t) v.emit_prune_lds(cutcap), nav->dp, b, cutcap);
		}
		else {
			launch_timed(nav, T_EF, st, true, v.emit_finish, grid, block, 0, nav->dp, b);
			launch_timed(nav, T_PM, st, true, k_prune_merge, grid, block, lp, nav->dp, b, cutcap);
		}
		if (with_alpha) {
			launch_timed(nav, T_WA, st, true, v.assoc, grid, block, la, nav->dp, b, cutcap);
			launch_timed(nav, T_WD, st, true, k_alpha_density, grid, block, 0, nav->dp, b);
		}
	}
	for (int s = 1; s < S && pipe < 0; s++) {
		HC(hipEventRecord(nav->ev_join[s - 1], nav->aux[s - 1]));
		HC(hipStreamWaitEvent(nav->stream, nav->ev_join[s - 1], 0));
	}
	HC(hipGetLastError());
	return PHD_OK;
}

// PHDNavigator.QuasiSetLogLikelihood (PHDNavigator.cs:526-531) for a batch of candidate poses against one landmark
// set and one measurement set: one workgroup per pose through the association kernel's own code.
int launch_quasi(phd_navigator* nav, const StepBufs& b, int nposes, bool gradient)
{
	const StepVariant& v = variant(b.M, false);
	hipLaunchKernelGGL(gradient ? v.quasi_grad : v.quasi, dim3(nposes), dim3(256), (size_t) v.assoc_lds(nav->cutcap), nav->stream, nav->dp, b, nav->cutcap);
	HC(hipGetLastError());
	return PHD_OK;
}

// graw / Pl / world (per-rank host): the weights still lie as the all-gather delivered them, [rank][Pl + 1]; the first launch un-gathers them
// pgp != NULL (sharded step whose plan runs over the grid too): the resampling's last launch also counts for the plan (*counted <- true)
int launch_normalise(phd_navigator* nav, const StepBufs& b, double* gw, int P, double u, int force, int skipnorm, int* src, int* info,
                     int* sel_next = nullptr, hipStream_t st = nullptr, const double* graw = nullptr, int Pl = 0, int world = 0,
                     const PlanGrid* pgp = nullptr, int rank = 0, const double* gflags = nullptr, bool* counted = nullptr)
{
	if (!st) st = nav->stream;
	if (nav->nr_grid_min > 0 && P >= nav->nr_grid_min && P <= 65536) {
		// one particle per thread over a grid, four launches (phd_resample.h, "over a GRID"): 16 384 weights in ~15 us instead of 48
		if (P > nav->nrcap) {
			HC(hipDeviceSynchronize());   // (first use, or a longer vector than ever before: rare)
			nav->d_nrd.reset(); nav->d_nri.reset();
			nav->nrcap = 0;
			const int Gc = (P + 255) / 256;
			HC(nav->d_nrd.alloc((size_t) Gc * (NR_STAT + NR_SLOT) + 2 * (size_t) P));
			HC(nav->d_nri.alloc((size_t) P + 4));
			nav->nrcap = P;
		}
		NrGrid nr;
		nr.G = (P + 255) / 256;
		nr.part = nav->d_nrd;
		nr.slotres = nr.part + (size_t) nr.G * NR_STAT;
		nr.pre = nr.slotres + (size_t) nr.G * NR_SLOT;
		nr.hi = nav->d_nri;
		nr.state = nav->d_nri + P;
		const int fr = nav->frozen ? 1 : 0;
		hipLaunchKernelGGL(k_nr_sum, dim3(nr.G), dim3(256), 0, st, b, gw, P, skipnorm, sel_next, nr, graw, Pl, world);
		hipLaunchKernelGGL(k_nr_stats, dim3(nr.G), dim3(256), 0, st, b, gw, P, skipnorm, sel_next, nr);
		hipLaunchKernelGGL(k_nr_slots, dim3(nr.G), dim3(256), 0, st, b, gw, P, nav->dp.min_eff, u, force, src, info, sel_next, fr, nav->d_inslot, nr);
		PlanGrid pgn;
		std::memset(&pgn, 0, sizeof pgn);
		if (pgp) { pgn = *pgp; if (counted) *counted = true; }
		hipLaunchKernelGGL(k_nr_sources, dim3(nr.G), dim3(256), 0, st, b, gw, P, u, src, info, sel_next, fr, nav->d_inslot, nr, pgn, Pl > 0 ? Pl : P, world > 0 ? world : 1,
		                   rank, gflags);
		HC(hipGetLastError());
		return PHD_OK;
	}
	if (graw) hipLaunchKernelGGL(k_ungather, dim3((P + world + 255) / 256), dim3(256), 0, st, graw, gw, Pl, world);
	// one workgroup; 256 / 512 threads for shorter weight vectors (fewer waves to meet at every barrier), 1024 beyond 4096
	const int nthreads = P <= 512 ? 256 : (P <= 4096 ? 512 : 1024);
	// the weight vector is staged in LDS (chunk-transposed: a whole chunk per thread, used or not) when it fits beside the
	// kernel's static arrays (160 KB per CU); above that the kernel works on the vector in global memory
	size_t lds = (size_t) ((P + nthreads - 1) / nthreads) * (nthreads + 1) * 8;
	int use_lds = lds + (size_t) nav->nr_static_lds + 256 <= 160 * 1024;
	if (!use_lds) lds = 0;
	hipLaunchKernelGGL(k_normalise_resample, dim3(1), dim3(nthreads), lds, st, b, gw, P, nav->dp.min_eff, u, force, skipnorm,
	                   use_lds, src, info, sel_next, nav->frozen ? 1 : 0, nav->d_inslot);
	HC(hipGetLastError());
	return PHD_OK;
}

int check_flags(phd_navigator* nav)
{
	int f = nav->h_flags;
	if (f & PHD_FLAG_EMIT_OVERFLOW) {
		return nav->fail(PHD_ERR_CAPACITY, "corrected mixture outgrew emit_capacity (" + std::to_string(nav->ecap) + " components per particle)");
	}
	if (f & PHD_FLAG_J_OVERFLOW) {
		return nav->fail(PHD_ERR_CAPACITY, "map estimate larger than the landmark scratch (" + std::to_string(nav->Jcap) + ")");
	}
	if (f & PHD_FLAG_ORDER_TIMEOUT) {
		return nav->fail(PHD_ERR_GENERIC, "a kernel gave up a bounded wait on the device: a helper workgroup of the one-launch chain for its particle's main workgroup (2 s; "
		                 "the step was dropped, the state is the one before it), or for the landing flag of a peer's migrating particles (phd_migration_set_landing: "
		                 "PHD_LANDING_TIMEOUT_MS; a rank has died, the state of this handle is undefined)");
	}
	if (f & PHD_FLAG_BIG_CLUSTER) {
		return nav->fail(PHD_ERR_ASSOCIATION, "a data-association cluster has more than " + std::to_string(MURTY_NBIG) + " rows, or the clusters beyond " +
		                 std::to_string(MURTY_NMAX) + " rows used up the association workspace (" + std::to_string(nav->bigws_bytes >> 20) +
		                 " MiB, phd_set_association_workspace); the step was dropped, the state is the one before it");
	}
	return PHD_OK;
}

// a component record -> the ABI's w, mean[3], cov[9] (row-major, the full symmetric matrix)
void unpack_record(const double* r, double* w, double* m, double* C)
{
	*w = r[0];
	for (int k = 0; k < 3; k++) m[k] = r[1 + k];
	const double xx = r[4], xy = r[5], xz = r[6], yy = r[7], yz = r[8], zz = r[9];
	C[0] = xx; C[1] = xy; C[2] = xz; C[3] = xy; C[4] = yy; C[5] = yz; C[6] = xz; C[7] = yz; C[8] = zz;
}

// copy one particle's mixture into h_mw / h_mm / h_mc (row-major mean[3n], cov[9n]): its count from the bank of the small
// arrays, its components from `mixbank` at the slot dslots[particle] (device array; NULL or the same bank: its own slot)
int fetch_map(phd_navigator* nav, int bankidx, int particle, int* ncomp, int mixbank = -1, const int* dslots = nullptr)
{
	int n = 0, slot = particle;
	HC(hipMemcpyAsync(&n, nav->bank[bankidx].count + particle, sizeof(int), hipMemcpyDeviceToHost, nav->stream));
	if (mixbank >= 0 && mixbank != bankidx && dslots) {
		HC(hipMemcpyAsync(&slot, dslots + particle, sizeof(int), hipMemcpyDeviceToHost, nav->stream));
	}
	HC(hipStreamSynchronize(nav->stream));
	if (slot < 0 || slot >= nav->Pcap) return nav->fail(PHD_ERR_GENERIC, "corrupt particle slot");
	const int srcbank = (mixbank >= 0) ? mixbank : bankidx;
	if (n < 0 || n > nav->cap) return nav->fail(PHD_ERR_GENERIC, "corrupt component count");
	nav->h_tmp.resize((size_t) MIX_REC * std::max(n, 1));
	if (n > 0) {   // the particle's records are one contiguous piece of its bank
		HC(hipMemcpyAsync(nav->h_tmp.data(), nav->bank[srcbank].mix + (size_t) slot * nav->cap * MIX_REC, (size_t) n * MIX_REC * 8,
		                  hipMemcpyDeviceToHost, nav->stream));
		HC(hipStreamSynchronize(nav->stream));
	}
	nav->h_mw.resize(std::max(n, 1));
	nav->h_mm.resize((size_t) 3 * std::max(n, 1));
	nav->h_mc.resize((size_t) 9 * std::max(n, 1));
	const double* t = nav->h_tmp.data();
	for (int c = 0; c < n; c++) unpack_record(t + (size_t) c * MIX_REC, &nav->h_mw[c], &nav->h_mm[(size_t) c * 3], &nav->h_mc[(size_t) c * 9]);
	*ncomp = n;
	return PHD_OK;
}

// host arrays -> the component records of one particle (covariance: upper triangle of the given 3x3)
void pack_records(const double* w, const double* mean3, const double* cov9, int n, double* recs)
{
	static const int tri[6] = {0, 1, 2, 4, 5, 8};
	for (int c = 0; c < n; c++) {
		double* r = recs + (size_t) c * MIX_REC;
		r[0] = w[c];
		for (int k = 0; k < 3; k++) r[1 + k] = mean3[c * 3 + k];
		for (int k = 0; k < 6; k++) r[4 + k] = cov9[c * 9 + tri[k]];
	}
}

int upload_particle(phd_navigator* nav, int bankidx, int particle, const double* w, const double* mean3,
                    const double* cov9, int n)
{
	if (n < 0 || n > nav->cap) return nav->fail(PHD_ERR_CAPACITY, "map larger than max_components");
	if (n > 0) {
		std::vector<double> recs((size_t) MIX_REC * n);
		pack_records(w, mean3, cov9, n, recs.data());
		HC(hipMemcpy(nav->bank[bankidx].mix + (size_t) particle * nav->cap * MIX_REC, recs.data(), (size_t) n * MIX_REC * 8, hipMemcpyHostToDevice));
	}
	HC(hipMemcpy(nav->bank[bankidx].count + particle, &n, sizeof(int), hipMemcpyHostToDevice));
	return PHD_OK;
}

int sync_state(phd_navigator* nav)
{
	HC(hipMemcpyAsync(nav->h_status, nav->d_sel, (2 * SEL_STRIDE + 3) * sizeof(int), hipMemcpyDeviceToHost, nav->stream));
	HC(hipStreamSynchronize(nav->stream));
	std::memcpy(nav->h_sel, nav->h_status + nav->parity * SEL_STRIDE, SEL_STRIDE * sizeof(int));
	std::memcpy(nav->h_info, nav->h_status + 2 * SEL_STRIDE, 2 * sizeof(int));
	nav->h_flags = nav->h_status[2 * SEL_STRIDE + 2];
	nav->sel_host_valid = true;
	return PHD_OK;
}

int cur_bank(const phd_navigator* nav) { return nav->h_sel[SEL_IN]; }

// Where the state a getter reports lives: the small arrays' bank, the mixtures' bank and the slot array. In frozen mode
// the roles do not advance and the result of the last step is described by RES / RESMIX and the resampling sources.
int res_small(const phd_navigator* nav) { return nav->frozen ? nav->h_sel[SEL_RES] : nav->h_sel[SEL_IN]; }
int res_mix(const phd_navigator* nav) { return nav->frozen ? nav->h_sel[SEL_RESMIX] : nav->h_sel[SEL_INMIX]; }
const int* res_slots(const phd_navigator* nav) { return nav->frozen ? (nav->d_res_slots ? nav->d_res_slots : nav->d_src) : nav->d_inslot; }

// The current state is about to be replaced as a whole: its mixtures will be addressed by particle number again.
int reset_indirection(phd_navigator* nav)
{
	std::vector<int> id(nav->Pcap);
	for (int i = 0; i < nav->Pcap; i++) id[i] = i;
	HC(hipMemcpy(nav->d_inslot, id.data(), (size_t) nav->Pcap * 4, hipMemcpyHostToDevice));
	nav->h_sel[SEL_INMIX] = nav->h_sel[SEL_IN];
	nav->h_sel[SEL_RES] = nav->h_sel[SEL_IN];
	nav->h_sel[SEL_RESMIX] = nav->h_sel[SEL_IN];
	HC(hipMemcpy(nav->d_sel + nav->parity * SEL_STRIDE, nav->h_sel, SEL_STRIDE * sizeof(int), hipMemcpyHostToDevice));
	return PHD_OK;
}

// Gather the mixtures of the current state into its own bank (k_materialise) if the last step left them behind an
// indirection. Needs the host mirror of the roles (sync_state).
int materialise(phd_navigator* nav)
{
	if (nav->h_sel[SEL_INMIX] == nav->h_sel[SEL_IN] || nav->P < 1) return PHD_OK;
	StepBufs b = make_bufs(nav);
	hipLaunchKernelGGL(k_materialise, dim3(nav->P), dim3(256), 0, nav->stream, b, nav->d_inslot);
	HC(hipGetLastError());
	HC(hipStreamSynchronize(nav->stream));
	nav->h_sel[SEL_INMIX] = nav->h_sel[SEL_IN];   // RES / RESMIX keep describing the last (frozen) step's result, which this did not touch
	HC(hipMemcpy(nav->d_sel + nav->parity * SEL_STRIDE, nav->h_sel, SEL_STRIDE * sizeof(int), hipMemcpyHostToDevice));
	return PHD_OK;
}

// The trajectory log starts again: no entries, pend the clean identity (on the handle's stream, behind whatever still reads it).
int hist_restart(phd_navigator* nav)
{
	nav->hist_len = 0;
	nav->h_htimes.clear(); nav->h_hmark.clear();
	if (nav->hist_cap < 1) return PHD_OK;
	nav->hist_pp ^= 1;
	hipLaunchKernelGGL(k_hist_identity, dim3((nav->Pcap + 255) / 256), dim3(256), 0, nav->stream, nav->hpend(nav->hist_pp), nav->hpdirty(nav->hist_pp), nav->Pcap);
	HC(hipGetLastError());
	return PHD_OK;
}

// The map log starts again: no entries, no records used (on the handle's stream, behind whatever still reads it).
int mlog_restart(phd_navigator* nav)
{
	nav->mlog_len = 0;
	nav->mlog_epoch++;
	nav->h_mltimes.clear();
	if (nav->mlog_cap < 1) return PHD_OK;
	HC(hipMemsetAsync(nav->d_mlbump, 0, 2 * sizeof(long long), nav->stream));
	return PHD_OK;
}

// ... both logs (phd_reset, phd_upload_state_soa)
int logs_restart(phd_navigator* nav)
{
	const int rc = hist_restart(nav);
	return rc ? rc : mlog_restart(nav);
}

// Behind the end of a step, on the stream that ran it: the step's resampling (if it had one and was not dropped) goes into pend.
int hist_compose(phd_navigator* nav, hipStream_t st)
{
	const int o = nav->hist_pp, n = o ^ 1;
	hipLaunchKernelGGL(k_hist_compose, dim3((nav->P + 255) / 256), dim3(256), 0, st, (const int*) nav->d_flags, (const int*) nav->d_info, (const int*) nav->d_src,
	                   (const int*) nav->hpend(o), (const int*) nav->hpdirty(o), nav->hpend(n), nav->hpdirty(n), nav->P);
	HC(hipGetLastError());
	nav->hist_pp = n;
	return PHD_OK;
}

}  // namespace

// ---- multi-device handle (phd_create_multi, phd_multi.inc): every entry point that means something for it dispatches here
int multi_reset(phd_navigator* nav, int nparticles, const double* pose7, const double* w, const double* mean3, const double* cov9, int ncomp);
int multi_set_small(phd_navigator* nav, const double* poses7, const double* weights, int nparticles);
int multi_update_motion(phd_navigator* nav, const double* odometry6, const double* noise6, int nparticles, uint8_t perfect_still);
int multi_set_map(phd_navigator* nav, int particle, const double* w, const double* mean3, const double* cov9, int ncomp);
int multi_upload(phd_navigator* nav, int nparticles, int stride, const double* planes, const int32_t* counts, const double* poses7, const double* weights);
int multi_download(phd_navigator* nav, int stride, double* planes, int32_t* counts, double* poses7, double* weights);
int multi_set_measurements(phd_navigator* nav, const double* z3, int nmeasurements);
int multi_set_depth_map(phd_navigator* nav, const float* depth, int width, int height);
int multi_step(phd_navigator* nav, uint8_t onlymapping, double u_resample);
int multi_sync(phd_navigator* nav);
int multi_forward_int(phd_navigator* nav, int what, long long value);
const double* multi_weights(phd_navigator* nav, int* length);
const double* multi_poses(phd_navigator* nav, int* length);
int multi_best_particle(phd_navigator* nav);
int multi_map(phd_navigator* nav, int particle, int* ncomp, const double** w, const double** mean3, const double** cov9);
const int32_t* multi_resample_sources(phd_navigator* nav, int* length, uint8_t* resampled);
void multi_destroy(phd_navigator* nav);
phd_navigator* multi_shard0(phd_navigator* nav);
static void multi_timing_reset(phd_navigator* nav, uint8_t enabled);
#define MULTI_UNSUPPORTED(nav, what) if ((nav) && (nav)->multi) return (nav)->fail(PHD_ERR_BAD_ARGUMENT, what ": not available on a multi-device handle (use a single-device handle)")
#define HISTORY_UNSUPPORTED(nav, what) if ((nav) && ((nav)->hist_cap > 0 || (nav)->mlog_cap > 0)) return (nav)->fail(PHD_ERR_BAD_ARGUMENT, (nav)->hist_cap > 0 ? \
	what ": not available while the trajectory log is on (phd_history_enable(nav, 0) switches it off; sharded ancestry is not kept)" : \
	what ": not available while the map log is on (phd_map_history_enable(nav, 0, 0) switches it off; the best particle may live on another shard)")

// =================================================================================================
extern "C" {

int phd_api_version(void) { return PHD_API_VERSION; }

const char* phd_create_error(void) { return g_create_error.c_str(); }

void phd_default_params(phd_params* p, int max_particles, int max_components, int max_measurements)
{
	std::memset(p, 0, sizeof(*p));
	p->model = PHD_MODEL_PRM3D;
	p->zdim  = 3;
	const double meas[7] = {575.8156, (double) 0.1f, (double) 2.0f, -320, -240, 640, 480};   // PRM3DMeasurer.cs:70-73
	std::memcpy(p->measurer, meas, sizeof(meas));
	p->R[0] = 2.0; p->R[4] = 2.0; p->R[8] = 1e-3;                                             // Config.cs:251-253
	for (int i = 0; i < 3; i++) p->visibility_ramp[i] = 3 * std::sqrt(p->R[i * 4]);          // Config.cs:257-259
	p->pd = 0.9;                                                                              // Config.cs:63,90
	p->clutter_density = 3e-7;                                                                // Config.cs:256,262
	p->birth_covariance[0] = p->birth_covariance[4] = p->birth_covariance[8] = 1e-2;          // Config.cs:77-79
	p->birth_weight = 0.05; p->min_weight = 1e-3; p->min_effective_particle = 0.1;            // Config.cs:80-82
	p->max_quantity = 600; p->merge_threshold = 0.3; p->exploration_threshold = 1e-5;         // Config.cs:83-85
	p->density_distance_threshold = 0.5;                                                      // Config.cs:74
	p->gate_metric = PHD_GATE_SQUARED_EUCLIDEAN;
	p->max_particles = max_particles; p->max_components = max_components; p->max_measurements = max_measurements;
	p->emit_capacity = 0;
}

phd_navigator* phd_create(const phd_params* params, int device)
{
	g_create_error.clear();
	if (!params) { g_create_error = "params is NULL"; return nullptr; }
	if (!((params->model == PHD_MODEL_PRM3D && params->zdim == 3) || (params->model == PHD_MODEL_LINEAR2D && params->zdim == 2))) {
		g_create_error = "model / zdim must be PRM3D / 3 or LINEAR2D / 2";
		return nullptr;
	}
	if (params->max_particles < 1 || params->max_components < 1 || params->max_measurements < 0 ||
	    params->max_measurements > 256 || params->max_quantity < 1 || params->max_components < params->max_quantity) {
		g_create_error = "capacities out of range (need max_components >= max_quantity >= 1, max_measurements <= 256)";
		return nullptr;
	}
	{
		// k_prune_merge and k_alpha_assoc keep their per-particle working set in LDS (160 KB per CU)
		const int zb = zb_of(params->max_measurements);
		const size_t need = std::max((size_t) prune_lds(params->max_quantity).bytes, (size_t) alpha_lds(zb * 64, params->max_quantity).bytes);
		if (need > 160 * 1024 - 512) {
			g_create_error = "max_quantity too large: pruning one particle needs " + std::to_string(need) + " bytes of LDS (160 KB per CU; about 3400 components fit)";
			return nullptr;
		}
	}
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
		g_create_error = "no HIP device: libphdhip has no CPU path";
		return nullptr;
	}
	if (device < 0 || device >= ndev || device >= PHD_MAX_DEVICES || hipSetDevice(device) != hipSuccess) {
		g_create_error = "bad device ordinal";
		return nullptr;
	}
	phd_navigator* nav = new phd_navigator();
	nav->prm = *params;
	nav->dp  = make_dev_params(*params);
	nav->device = device;
	nav->Pcap = params->max_particles;
	nav->cap  = (params->max_components + 63) & ~63;
	nav->Mcap = std::max(64, (params->max_measurements + 63) & ~63);
	nav->cutcap = params->max_quantity;
	int ecap = params->emit_capacity > 0 ? params->emit_capacity : 4 * (nav->cap + nav->Mcap);
	nav->ecap = (std::max(ecap, nav->cutcap) + 63) & ~63;
	nav->Jcap = std::min(1024, (nav->cutcap + 63) & ~63);
	nav->P = 0;

	auto dalloc = [](auto& buf, size_t bytes) {   // (at least 16 bytes; every size here is a whole number of the buffer's elements)
		const size_t el = sizeof(typename std::remove_reference_t<decltype(buf)>::element);
		return buf.alloc((std::max<size_t>(bytes, 16) + el - 1) / el) == hipSuccess;
	};
	bool ok = hipStreamCreateWithFlags(nav->own_stream.put(), hipStreamNonBlocking) == hipSuccess;
	nav->stream = nav->own_stream;
	// The events that order the sub-range streams among themselves (same device, never inspected by the host): recorded without
	// the system-scope fence a default event performs (5 us per step boundary; the kernels' own release / acquire at their ends
	// and starts is what the next stream's kernels see). PHD_EVENT_FLAGS=0: default events.
	unsigned evflags = hipEventDisableTiming | hipEventDisableSystemFence;
	if (const char* e = getenv("PHD_EVENT_FLAGS")) {
		const int m = atoi(e);
		if (m == 0) evflags = hipEventDisableTiming;
		if (m == 1) evflags = hipEventDisableTiming | hipEventReleaseToDevice;
	}
	// (a runtime that refuses the fence-less flag gets plain untimed events: slower boundaries, the same order)
	auto ev_create = [&](hipEvent_t* ev, unsigned flags) {
		if (hipEventCreateWithFlags(ev, flags) == hipSuccess) return true;
		(void) hipGetLastError();
		return hipEventCreateWithFlags(ev, hipEventDisableTiming) == hipSuccess;
	};
	for (int i = 0; i < phd_navigator::MAXSPLIT - 1; i++) {
		ok = ok && hipStreamCreateWithFlags(nav->aux[i].put(), hipStreamNonBlocking) == hipSuccess;
		ok = ok && ev_create(nav->ev_join[i].put(), evflags);
	}
	// ev_fork keeps the default (system-scope) release: it is recorded exactly when something ELSE preceded the step on the
	// handle's stream — typically the host-to-device copy of phd_set_measurements — and is then the only link between that copy
	// and the aux stream's k_sweep. It is off the back-to-back path (phd_step_async behind phd_step_async records no fork), so its
	// 5 us do not touch the steady state.
	ok = ok && ev_create(nav->ev_fork.put(), hipEventDisableTiming);
	ok = ok && ev_create(nav->ev_res.put(), evflags);
	if (const char* e = getenv("PHD_PIPELINE")) nav->pipeline = atoi(e) != 0;
	if (const char* e = getenv("PHD_FUSE_EP")) nav->fuse_ep = atoi(e) != 0 ? 1 : 0;
	if (const char* e = getenv("PHD_SPLIT")) nav->nsplit = std::max(0, atoi(e));
	if (const char* e = getenv("PHD_CHAIN_MAX")) nav->chain_max = std::max(0, atoi(e));
	if (const char* e = getenv("PHD_DSPLIT_MAX")) nav->dsplit_max = std::max(0, atoi(e));
	if (const char* e = getenv("PHD_DSPLIT_LATE")) nav->dsplit_late = atoi(e);
	if (const char* e = getenv("PHD_DSPLIT_SEQ0")) nav->dseq = (unsigned int) std::max(0LL, atoll(e));   // (tests: launch numbers that start again soon)
	if (const char* e = getenv("PHD_NR_GRID_MIN")) nav->nr_grid_min = std::max(0, atoi(e));
	if (const char* e = getenv("PHD_PLAN_GRID_MIN")) nav->plan_grid_min = std::max(0, atoi(e));
	size_t plane = (size_t) nav->Pcap * nav->cap;
	for (int i = 0; i < 3 && ok; i++) {
		ok = ok && dalloc(nav->bank_mix[i], plane * MIX_REC * 8);
		ok = ok && dalloc(nav->bank_count[i], (size_t) nav->Pcap * 4);
		ok = ok && dalloc(nav->bank_poses[i], (size_t) nav->Pcap * 7 * 8);
		ok = ok && dalloc(nav->bank_weights[i], (size_t) nav->Pcap * 8);
		nav->bank[i] = Bank{nav->bank_mix[i], nav->bank_count[i], nav->bank_poses[i], nav->bank_weights[i]};
		if (ok) {
			hipMemset(nav->bank[i].count, 0, (size_t) nav->Pcap * 4);
			hipMemset(nav->bank[i].weights, 0, (size_t) nav->Pcap * 8);
			hipMemset(nav->bank[i].poses, 0, (size_t) nav->Pcap * 7 * 8);
		}
	}
	size_t E = (size_t) nav->Pcap * nav->ecap;
	// the role tables (two parities), the step's info words and its flag word in ONE block: phd_sync reads it with one copy
	// queued on the stream it then waits for (three blocking copies before: 40 us of a 90 us step at config A)
	ok = ok && dalloc(nav->d_sel, (2 * SEL_STRIDE + 4) * 4) && dalloc(nav->d_inslot, (size_t) nav->Pcap * 4);
	if (ok) { nav->d_info = nav->d_sel + 2 * SEL_STRIDE; nav->d_flags = nav->d_info + 2; }
	ok = ok && nav->h_status.alloc(2 * SEL_STRIDE + 4, hipHostMallocDefault) == hipSuccess;
	ok = ok && dalloc(nav->d_z, (size_t) nav->Mcap * 3 * 8);
	ok = ok && dalloc(nav->d_emit_w, E * 8) && dalloc(nav->d_emit_idx, E * 4);
	ok = ok && dalloc(nav->d_emit_rec, E * MIX_REC * 8) && dalloc(nav->d_emit_count, (size_t) nav->Pcap * 4);
	ok = ok && dalloc(nav->d_born_count, (size_t) nav->Pcap * 4);
	ok = ok && dalloc(nav->d_born_k, (size_t) nav->Pcap * nav->Mcap * 4);
	ok = ok && dalloc(nav->d_born_mean, (size_t) nav->Pcap * nav->Mcap * 3 * 8);
	ok = ok && dalloc(nav->d_alpha, (size_t) nav->Pcap * 8) && dalloc(nav->d_setll, (size_t) nav->Pcap * 8);
	ok = ok && dalloc(nav->d_src, (size_t) nav->Pcap * 4);
	ok = ok && dalloc(nav->d_murty, (size_t) nav->Pcap * sizeof(MurtyNodes));
	nav->bigws_bytes = 128ull << 20;
	ok = ok && dalloc(nav->d_bigws, nav->bigws_bytes) && dalloc(nav->d_bigws_used, 8);   // the slab's bump counter
	if (ok) hipMemset(nav->d_bigws_used, 0, 8);
	nav->cmcap = nav->cap + nav->Mcap;
	ok = ok && dalloc(nav->d_cand_count, (size_t) nav->Pcap * 4 * 4) && dalloc(nav->d_denom, (size_t) nav->Pcap * nav->Mcap * 8);
	nav->candcap = 16 * nav->cmcap;   // a quarter of all pairs at 64 measurements (four wave segments); beyond it the full second sweep runs
	ok = ok && dalloc(nav->d_cand, (size_t) nav->Pcap * nav->candcap * 8);
#ifdef PHD_STAMPS
	ok = ok && dalloc(nav->d_stamps, (size_t) nav->Pcap * 16 * 8);
#endif
	ok = ok && dalloc(nav->d_srec, (size_t) nav->Pcap * PRUNE_ROW * nav->cutcap * 8);
	ok = ok && dalloc(nav->d_outw, plane * 8);
	ok = ok && dalloc(nav->d_ratio, (size_t) nav->Pcap * 8);
	ok = ok && dalloc(nav->d_wcopy, (size_t) nav->Pcap * (nav->cap + nav->Mcap) * 8) && dalloc(nav->d_cover, (size_t) nav->Pcap * nav->cap * 4);
	ok = ok && dalloc(nav->d_alm, (size_t) nav->Pcap * 3 * nav->Jcap * 8);
	ok = ok && dalloc(nav->d_aJ, (size_t) nav->Pcap * 4) && dalloc(nav->d_account, (size_t) nav->Pcap * 8);
	if (nav->dsplit_max > 0) {
		const size_t rows = (size_t) std::min(nav->Pcap, (int) DSPLIT_ROWS);
		ok = ok && dalloc(nav->d_dsync, rows * 3 * 4);
		ok = ok && hipMemset(nav->d_dsync, 0, rows * 3 * 4) == hipSuccess;
	}
	ok = ok && dalloc(nav->d_jscratch, (size_t) nav->Pcap * alpha_jscratch_doubles(nav->Jcap) * 8);
	nav->stagecap = std::max((size_t) nav->Pcap * 8 + 8, (size_t) 256 * 3);   // poses + weights | odometry + noise | measurements
	ok = ok && dalloc(nav->d_stage, nav->stagecap * 8) && dalloc(nav->d_motion, ((size_t) nav->Pcap * 6 + 6) * 8);
	for (int i = 0; i < 2; i++) {
		ok = ok && nav->h_stage[i].alloc(nav->stagecap, hipHostMallocDefault) == hipSuccess;
		ok = ok && hipEventCreateWithFlags(nav->ev_stage[i].put(), hipEventDisableTiming) == hipSuccess;
	}
	{
		// dynamic LDS limits, set when a handle is created: they depend on the handle's capacities only. The attribute belongs
		// to the function ON THE CURRENT DEVICE, and the same kernels serve every handle of the process there: per device
		// the limit is only ever raised.
		struct DevLimits { int prune = 0, alpha[8] = {0, 0, 0, 0, 0, 0, 0, 0}, chain[8] = {0, 0, 0, 0, 0, 0, 0, 0}; };   // (per row of step_variants)
		static DevLimits limits[PHD_MAX_DEVICES];
		static std::mutex limits_mu;   // (handles may be created from several host threads, one per GPU)
		std::lock_guard<std::mutex> limits_guard(limits_mu);
		DevLimits& lim = limits[device];
		auto raise = [&](auto kernel, int bytes) { ok = ok && hipFuncSetAttribute((const void*) kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess; };
		const int cutcap = nav->cutcap, lp = prune_lds(cutcap).bytes;
		const bool raise_prune = lp > lim.prune;
		if (raise_prune) raise(k_prune_merge, lp);
		for (int z = 0; z < 3; z++) nav->chain_ok[z] = true;
		for (int i = 0; i < 8; i++) {
			const StepVariant& v = step_variants[i];
			if (raise_prune) raise(v.emit_prune, v.emit_prune_lds(cutcap));
			const int la = v.assoc_lds(cutcap);
			if (la > lim.alpha[i]) {
				raise(v.assoc, la);
				raise(v.quasi, la);
				raise(v.quasi_grad, la);
				raise(v.ascent, la);
				raise(v.ascent_grad, la);
				raise(v.multi, la);
				raise(v.multi_grad, la);
				lim.alpha[i] = la;
			}
			// the one-launch chain: its bodies share one pool, the largest of their layouts, which must fit a workgroup (160 KB)
			// with the kernel's few static words; where it does not (a large MaxQuantity) the separate kernels run. A step runs
			// the chain only where every build it could pick at its ZB fits (with and without a depth map, HALF or not).
			const int lc = v.chain_lds(cutcap);
			hipFuncAttributes fc;
			bool fits = false;
			if (!ok || hipFuncGetAttributes(&fc, (const void*) v.chain) != hipSuccess) ok = false;
			else if ((size_t) fc.sharedSizeBytes + (size_t) lc + 256 <= 160 * 1024) {
				if (lc <= lim.chain[i]) fits = true;
				else if (hipFuncSetAttribute((const void*) v.chain, hipFuncAttributeMaxDynamicSharedMemorySize, lc) == hipSuccess) { lim.chain[i] = lc; fits = true; }
				else (void) hipGetLastError();   // (a build that does not fit is skipped, not an error)
			}
			if (!fits) nav->chain_ok[v.zi()] = false;
		}
		if (raise_prune) lim.prune = lp;
		ok = ok && hipFuncSetAttribute((const void*) k_plan_migration, hipFuncAttributeMaxDynamicSharedMemorySize, PLAN_LDS_MAX + 1024) == hipSuccess;
		hipFuncAttributes fa;
		if (ok && hipFuncGetAttributes(&fa, (const void*) k_normalise_resample) == hipSuccess) {
			nav->nr_static_lds = (int) fa.sharedSizeBytes;
			ok = ok && hipFuncSetAttribute((const void*) k_normalise_resample, hipFuncAttributeMaxDynamicSharedMemorySize,
			                               160 * 1024 - nav->nr_static_lds) == hipSuccess;
		}
		else ok = false;
	}
	if (!ok) {
		g_create_error = std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError());
		phd_destroy(nav);
		return nullptr;
	}
	int sel[2 * SEL_STRIDE] = {0, 1, 2, 0, 0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0};
	hipMemcpy(nav->d_sel, sel, sizeof(sel), hipMemcpyHostToDevice);
	{
		std::vector<int> id(nav->Pcap);
		for (int i = 0; i < nav->Pcap; i++) id[i] = i;
		hipMemcpy(nav->d_inslot, id.data(), (size_t) nav->Pcap * 4, hipMemcpyHostToDevice);
	}
	hipMemset(nav->d_flags, 0, 4);
	hipMemset(nav->d_info, 0, 8);
	hipMemset(nav->d_emit_count, 0, (size_t) nav->Pcap * 4);
	hipMemset(nav->d_born_count, 0, (size_t) nav->Pcap * 4);
	return nav;
}

void phd_destroy(phd_navigator* nav)
{
	if (!nav) return;
	if (nav->multi) { multi_destroy(nav); return; }
	enter(nav);
	if (nav->stream) hipStreamSynchronize(nav->stream);
	for (void* q : nav->ipc_opened) hipIpcCloseMemHandle(q);
	for (Timer& t : nav->timers) { hipEventDestroy(t.t0); hipEventDestroy(t.t1); }
	delete nav;   // (its owners release the buffers, events and streams; the device is current: enter)
}

const char* phd_last_error(const phd_navigator* nav) { return nav ? nav->err.c_str() : "null handle"; }

int phd_particle_count(phd_navigator* nav) { return nav ? nav->P : 0; }

// phd_reset with the particle weight given (a shard of a multi-device handle holds 1 / the TOTAL count)
static int reset_impl(phd_navigator* nav, int nparticles, const double* pose7, const double* w, const double* mean3,
                      const double* cov9, int ncomp, double weight)
{
	if (nparticles < 1 || nparticles > nav->Pcap || !pose7 || ncomp < 0) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_reset: bad particle count / pose / ncomp");
	enter(nav);
	int rc = sync_state(nav);
	if (rc) return rc;
	rc = reset_indirection(nav);   // the state is replaced as a whole
	if (rc) return rc;
	int I = nav->h_sel[SEL_IN];
	rc = upload_particle(nav, I, 0, w, mean3, cov9, ncomp);
	if (rc) return rc;
	HC(hipMemcpy(nav->bank[I].poses, pose7, 7 * 8, hipMemcpyHostToDevice));
	nav->P = nparticles;
	StepBufs b = make_bufs(nav);
	hipLaunchKernelGGL(k_replicate, dim3(nparticles), dim3(256), 0, nav->stream, b, weight);
	HC(hipGetLastError());
	// the replicated state is in the OUT bank: make it current
	const int O = nav->h_sel[SEL_OUT], T = nav->h_sel[SEL_TMP];
	int sel[SEL_STRIDE] = {O, I, T, O, O, O, 0, 0};   // IN, OUT, TMP, RES, INMIX, RESMIX
	HC(hipStreamSynchronize(nav->stream));
	HC(hipMemcpy(nav->d_sel + nav->parity * SEL_STRIDE, sel, sizeof(sel), hipMemcpyHostToDevice));
	std::memcpy(nav->h_sel, sel, sizeof(sel));
	nav->h_info[0] = 0; nav->h_info[1] = 0;   // BestParticle = 0 (:265)
	HC(hipMemcpy(nav->d_info, nav->h_info, 8, hipMemcpyHostToDevice));
	nav->stage_valid = false;
	return logs_restart(nav);
}

int phd_reset(phd_navigator* nav, int nparticles, const double* pose7, const double* w, const double* mean3,
              const double* cov9, int ncomp)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (ncomp > 0 && (!w || !mean3 || !cov9)) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_reset: map arrays are NULL");
	FINITE_OR_FAIL(nav, pose7, 7, "phd_reset");
	FINITE_OR_FAIL(nav, w, std::max(ncomp, 0), "phd_reset");
	FINITE_OR_FAIL(nav, mean3, (size_t) std::max(ncomp, 0) * 3, "phd_reset");
	FINITE_OR_FAIL(nav, cov9, (size_t) std::max(ncomp, 0) * 9, "phd_reset");
	if (nav->multi) return multi_reset(nav, nparticles, pose7, w, mean3, cov9, ncomp);
	return reset_impl(nav, nparticles, pose7, w, mean3, cov9, ncomp, 1.0 / std::max(nparticles, 1));
}

int phd_set_poses(phd_navigator* nav, const double* poses7, int nparticles)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nparticles != nav->P || !poses7) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_set_poses: particle count mismatch");
	FINITE_OR_FAIL(nav, poses7, (size_t) nparticles * 7, "phd_set_poses");
	if (nav->multi) return multi_set_small(nav, poses7, nullptr, nparticles);
	enter(nav);
	// the bank that holds the current poses is known to the device (the roles rotate there, at the end of a step): the poses
	// are staged and stored by a kernel that resolves it, so this is correct right behind phd_step_async and never waits
	double* hs = stage_acquire(nav);
	std::memcpy(hs, poses7, (size_t) nparticles * 7 * 8);
	HC(hipMemcpyAsync(nav->d_stage, hs, (size_t) nparticles * 7 * 8, hipMemcpyHostToDevice, nav->stream));
	stage_release(nav);
	StepBufs b = make_bufs(nav);
	hipLaunchKernelGGL(k_store_small, dim3((nparticles * 7 + 255) / 256), dim3(256), 0, nav->stream, b, (const double*) nav->d_stage, (const double*) nullptr, nparticles);
	HC(hipGetLastError());
	nav->stage_valid = false;
	return PHD_OK;
}

// TrackVehicle.UpdateNoisy for every particle, on the device: the host passes the odometry reading
// and, per particle, the noise vector it drew (RNG and Cholesky factor stay managed); no pose array crosses PCIe.
int phd_update_motion(phd_navigator* nav, const double* odometry6, const double* noise6, int nparticles, uint8_t perfect_still)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (!odometry6 || nparticles != nav->P) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_update_motion: particle count mismatch");
	FINITE_OR_FAIL(nav, odometry6, 6, "phd_update_motion");
	FINITE_OR_FAIL(nav, noise6, (size_t) nparticles * 6, "phd_update_motion");
	if (nav->multi) return multi_update_motion(nav, odometry6, noise6, nparticles, perfect_still);
	if (nav->prm.model != PHD_MODEL_PRM3D) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_update_motion: Pose3D odometry, the PRM3D model only");
	enter(nav);
	bool zero = true;
	for (int t = 0; t < 6; t++) zero = zero && odometry6[t] == 0;
	const int use_noise = noise6 && !(perfect_still && zero);   // "static friction makes the robot stay put", TrackVehicle.cs:93-94
	double* hs = stage_acquire(nav);
	std::memcpy(hs, odometry6, 6 * 8);
	if (use_noise) std::memcpy(hs + 6, noise6, (size_t) nparticles * 6 * 8);
	HC(hipMemcpyAsync(nav->d_motion, hs, (6 + (use_noise ? (size_t) nparticles * 6 : 0)) * 8, hipMemcpyHostToDevice, nav->stream));
	stage_release(nav);   // the caller's buffers are free again; nothing waits for the device
	StepBufs b = make_bufs(nav);
	hipLaunchKernelGGL(k_motion, dim3((nparticles + 255) / 256), dim3(256), 0, nav->stream, b, nparticles,
	                   (const double*) nav->d_motion, (const double*) (nav->d_motion + 6), use_noise);
	HC(hipGetLastError());
	nav->stage_valid = false;
	return PHD_OK;
}

static int quasi_batch(phd_navigator* nav, const double* poses7, int nposes, const double* landmarks3, int nlandmarks,
                       const double* z3, int nmeasurements, double* out, double* gradients6, int average_mode)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);   // a batch of candidate poses against one landmark set does not touch the particle state
	if (nposes < 1 || nposes > nav->Pcap || nlandmarks < 0 || nlandmarks > nav->Jcap || nmeasurements < 0 ||
	    nmeasurements > nav->prm.max_measurements || !poses7 || !out || (nlandmarks && !landmarks3) || (nmeasurements && !z3)) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_quasi_set_loglik: sizes out of range (poses <= max_particles, landmarks <= min(1024, max_quantity rounded up to 64), measurements <= max_measurements)");
	}
	FINITE_OR_FAIL(nav, poses7, (size_t) nposes * 7, "phd_quasi_set_loglik");
	FINITE_OR_FAIL(nav, landmarks3, (size_t) nlandmarks * 3, "phd_quasi_set_loglik");
	FINITE_OR_FAIL(nav, z3, (size_t) nmeasurements * 3, "phd_quasi_set_loglik");
	enter(nav);
	// One buffer on the device and its pinned mirror on the host, packed per call:
	//   poses[n][7] | landmarks[J][3] | z[M][3] | flag word | slab counter | out[n] | gradients[n][6]
	// so that a call is ONE copy in (inputs, with the two words zeroed), the kernel, ONE copy out (from the flag word on) and
	// one wait. The smoother calls this in a loop: six copies from and to pageable memory, two memsets and a blocking read of
	// the step's flag word cost more than the value kernel's 40 us. The batch has a flag word and a slab counter of its own:
	// nothing it raises can drop the next step, and the step's association kernel finds its counter as it left it.
	const size_t cap = (size_t) nav->Pcap * 14 + (size_t) nav->Jcap * 3 + 256 * 3 + 2;
	const size_t op = 0, ol = op + (size_t) nposes * 7, oz = ol + (size_t) nlandmarks * 3, of = oz + (size_t) nmeasurements * 3, ou = of + 1,
	             oo = ou + 1, og = oo + nposes, end = og + (gradients6 ? (size_t) nposes * 6 : 0);
	if (!nav->d_quasi) HC(nav->d_quasi.alloc(cap));
	if (!nav->h_quasi) HC(nav->h_quasi.alloc(cap, hipHostMallocDefault));
	double* const hq = nav->h_quasi;
	std::memcpy(hq + op, poses7, (size_t) nposes * 7 * 8);
	if (nlandmarks) std::memcpy(hq + ol, landmarks3, (size_t) nlandmarks * 3 * 8);
	if (nmeasurements) std::memcpy(hq + oz, z3, (size_t) nmeasurements * 3 * 8);
	hq[of] = 0; hq[ou] = 0;
	HC(hipMemcpyAsync(nav->d_quasi, hq, oo * 8, hipMemcpyHostToDevice, nav->stream));
	StepBufs b = make_bufs(nav);
	b.P = nposes; b.M = nmeasurements; b.z = nav->d_quasi + oz;
	b.qposes = nav->d_quasi + op; b.qlm = nav->d_quasi + ol; b.qJ = nlandmarks;
	b.setll = nav->d_quasi + oo;
	b.qgrad = nav->d_quasi + og;
	b.qavg  = average_mode;
	b.flags = (int*) (nav->d_quasi + of);
	b.bigws_used = (unsigned long long*) (nav->d_quasi + ou);
	const bool gradient = gradients6 != nullptr;
	const int rc = launch_quasi(nav, b, nposes, gradient);
	if (rc) return rc;
	HC(hipMemcpyAsync(hq + of, nav->d_quasi + of, (end - of) * 8, hipMemcpyDeviceToHost, nav->stream));
	HC(hipStreamSynchronize(nav->stream));
	std::memcpy(out, hq + oo, (size_t) nposes * 8);
	if (gradient) std::memcpy(gradients6, hq + og, (size_t) nposes * 6 * 8);
	int flags = 0;
	std::memcpy(&flags, hq + of, 4);
	if (flags & PHD_FLAG_BIG_CLUSTER) {
		return nav->fail(PHD_ERR_ASSOCIATION, "phd_quasi_set_loglik: an association cluster exceeds the on-device solver");
	}
	return PHD_OK;
}

int phd_quasi_set_loglik(phd_navigator* nav, const double* poses7, int nposes, const double* landmarks3, int nlandmarks,
                         const double* z3, int nmeasurements, double* out)
{
	return quasi_batch(nav, poses7, nposes, landmarks3, nlandmarks, z3, nmeasurements, out, nullptr, 0);
}

int phd_quasi_set_loglik_grad(phd_navigator* nav, const double* poses7, int nposes, const double* landmarks3, int nlandmarks,
                              const double* z3, int nmeasurements, int average_mode, double* out, double* gradients6)
{
	if (nav && (!gradients6 || average_mode < 0 || average_mode > 1)) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_quasi_set_loglik_grad: gradients6 is NULL or average_mode is not 0 / 1");
	}
	return quasi_batch(nav, poses7, nposes, landmarks3, nlandmarks, z3, nmeasurements, out, gradients6, average_mode);
}

// ---- phd_quasi_ascent: LogLikeGradientAscent resident on the device (phd_ascent.h) ----
namespace {

#define PHD_ASCENT_ROUND 2   // iterations enqueued between two looks at the active count (profiles/ascent_cost.md: searches end after 2 - 5)

// One buffer per handle, in doubles, sized once for the largest call (Pcap / 16 estimates, Jcap landmarks, 256 measurements):
//   lin[7] | landmarks[J][3] | z[M][3] | head[4] (flag word, slab counter, active count, spare) | pose6[n][6]      <- ONE copy in
//                                         head[4] | pose6[n][6] | loglike[n] | iterations[n] | hessians[n][36]     <- ONE copy out
// and behind them the state that never leaves the device. The inputs are packed per call, so `head` moves with J and M.
struct AscentLayout {
	size_t lin, lm, z, head, pose6, loglike, iters, hess, out_end, next7, prev, active, chosen, grad, gval, cand6, cand7, values, hpose, hgrad, hval, end;
};

AscentLayout ascent_layout(size_t n, size_t J, size_t M)
{
	AscentLayout l;
	l.lin = 0; l.lm = 7; l.z = l.lm + J * 3; l.head = l.z + M * 3; l.pose6 = l.head + 4;
	l.loglike = l.pose6 + n * 6; l.iters = l.loglike + n; l.hess = l.iters + n; l.out_end = l.hess + n * 36;
	l.next7 = l.out_end; l.prev = l.next7 + n * 7; l.active = l.prev + n; l.chosen = l.active + n; l.grad = l.chosen + n; l.gval = l.grad + n * 6;
	l.cand6 = l.gval + n; l.cand7 = l.cand6 + n * PHD_ASCENT_LINE * 6; l.values = l.cand7 + n * PHD_ASCENT_LINE * 7;
	l.hpose = l.values + n * PHD_ASCENT_LINE; l.hgrad = l.hpose + n * 12 * 7; l.hval = l.hgrad + n * 12 * 6; l.end = l.hval + n * 12;
	return l;
}

AscentBufs ascent_bufs(double* d, const AscentLayout& l, int n)
{
	AscentBufs s;
	s.n = n; s.lin = d + l.lin; s.problem = nullptr;
	s.flags = (int*) (d + l.head); s.slab = (unsigned long long*) (d + l.head + 1); s.nactive = (int*) (d + l.head + 2);
	s.pose6 = d + l.pose6; s.loglike = d + l.loglike; s.iterations = (int*) (d + l.iters); s.hess = d + l.hess;
	s.nextpose7 = d + l.next7; s.prev = d + l.prev; s.active = (int*) (d + l.active); s.chosen = (int*) (d + l.chosen);
	s.grad = d + l.grad; s.gval = d + l.gval; s.cand6 = d + l.cand6; s.cand7 = d + l.cand7; s.values = d + l.values;
	s.hpose = d + l.hpose; s.hgrad = d + l.hgrad; s.hval = d + l.hval;
	return s;
}

int ascent_ensure(phd_navigator* nav)
{
	if (nav->d_ascent && nav->h_ascent) return PHD_OK;
	const AscentLayout cap = ascent_layout((size_t) (nav->Pcap / PHD_ASCENT_LINE), (size_t) nav->Jcap, 256);
	HC(nav->d_ascent.alloc(cap.end));
	HC(nav->h_ascent.alloc(cap.end + 1, hipHostMallocDefault));   // (+ the word read between rounds)
	return PHD_OK;
}

// an evaluation launch of the chain: `nposes` poses at `poses7`, values to `setll`, gradients to `qgrad` (NULL: the value kernel)
int ascent_eval(phd_navigator* nav, const AscentBufs& s, const AscentLayout& l, int J, int M, int average_mode, const double* poses7, int nposes,
                double* setll, double* qgrad, const int* active, int group)
{
	StepBufs b = make_bufs(nav);
	b.P = nposes; b.M = M; b.z = nav->d_ascent + l.z;
	b.qposes = poses7; b.qlm = nav->d_ascent + l.lm; b.qJ = J;
	b.setll = setll; b.qgrad = qgrad; b.qavg = average_mode;
	b.flags = s.flags; b.bigws_used = s.slab;
	const StepVariant& v = variant(M, false);
	hipLaunchKernelGGL(qgrad ? v.ascent_grad : v.ascent, dim3(nposes), dim3(256), (size_t) v.assoc_lds(nav->cutcap), nav->stream, nav->dp, b, nav->cutcap, active, group);
	HC(hipGetLastError());
	return PHD_OK;
}

inline int ascent_blocks(int threads) { return (threads + 255) / 256; }

// The chain of one call, enqueued on the handle's stream: begin, the first gradient launch, the iterations in rounds with one
// look at the active count between two rounds, the Hessian rows. `eval(poses7, nposes, setll, qgrad, active, group)` launches an
// evaluation: phd_quasi_ascent's own (ascent_eval) or the one over many problems (multi_eval). `word`: pinned, for that look.
using AscentEval = std::function<int(const double*, int, double*, double*, const int*, int)>;
int ascent_chain(phd_navigator* nav, const AscentBufs& s, int max_iterations, int round_iterations, bool hessians, int* word, const AscentEval& eval)
{
	const int n = s.n;
	hipStream_t st = nav->stream;
	hipLaunchKernelGGL(k_ascent_begin, dim3(ascent_blocks(n)), dim3(256), 0, st, s);
	int rc = eval(s.nextpose7, n, s.gval, s.grad, nullptr, 1);
	if (rc) return rc;
	hipLaunchKernelGGL(k_ascent_start, dim3(ascent_blocks(n)), dim3(256), 0, st, s);
	const int round = round_iterations > 0 ? round_iterations : PHD_ASCENT_ROUND;
	int done = 0;
	while (done < max_iterations) {
		const int upto = std::min(max_iterations, done + round);
		for (; done < upto; done++) {
			if (done > 0) {   // (iteration 0 keeps the first launch's gradient: the same pose through the same kernel)
				rc = eval(s.nextpose7, n, s.gval, s.grad, s.active, 1);
				if (rc) return rc;
			}
			hipLaunchKernelGGL(k_ascent_candidates, dim3(ascent_blocks(n * PHD_ASCENT_LINE)), dim3(256), 0, st, s);
			rc = eval(s.cand7, n * PHD_ASCENT_LINE, s.values, nullptr, s.active, PHD_ASCENT_LINE);
			if (rc) return rc;
			hipLaunchKernelGGL(k_ascent_select, dim3(ascent_blocks(n)), dim3(256), 0, st, s);
		}
		if (done >= max_iterations) break;   // (the count comes with the results)
		HC(hipMemcpyAsync(word, s.nactive, 4, hipMemcpyDeviceToHost, st));
		HC(hipStreamSynchronize(st));
		if (*word == 0) break;
	}
	if (hessians) {
		hipLaunchKernelGGL(k_ascent_hess_poses, dim3(ascent_blocks(n * 12)), dim3(256), 0, st, s);
		rc = eval(s.hpose, n * 12, s.hval, s.hgrad, nullptr, 12);   // (12 poses per estimate: the group tells a launch over many problems whose pose it has)
		if (rc) return rc;
		hipLaunchKernelGGL(k_ascent_hess_rows, dim3(ascent_blocks(n * 36)), dim3(256), 0, st, s);
	}
	HC(hipGetLastError());
	return PHD_OK;
}

// ---- many problems in one call (phd_ascent_multi.h). One buffer per handle, grown to the largest call, in doubles (the int
// arrays two to a double):
//   lm_off[np + 1] | z_off[np + 1] | problem[n] | landmarks[sum J][3] | z[sum M][3] | lin[np][7] | head[4] | pose6[n][6]   <- ONE copy in
// and from `head` on what ascent_layout states: the copy out, then the state that never leaves the device. The batch calls put
// poses7[n][7] where lin stands and out[n] | gradients[n][6] behind head. The flag word and the slab counter in `head` are this
// buffer's own: the step and the single calls find theirs untouched.
struct MultiLayout {
	size_t lmoff, zoff, problem, lm, z, lin, head;
	AscentLayout a;   // ascent_layout's offsets from `head` on, within this buffer
};

MultiLayout multi_layout(size_t np, size_t n, size_t sumJ, size_t sumM, size_t lin_doubles)
{
	MultiLayout l;
	l.lmoff = 0; l.zoff = l.lmoff + (np + 2) / 2; l.problem = l.zoff + (np + 2) / 2; l.lm = l.problem + (n + 1) / 2;
	l.z = l.lm + sumJ * 3; l.lin = l.z + sumM * 3; l.head = l.lin + lin_doubles;
	l.a = ascent_layout(n, 0, 0);
	const size_t shift = l.head - l.a.head;
	for (size_t* f : {&l.a.head, &l.a.pose6, &l.a.loglike, &l.a.iters, &l.a.hess, &l.a.out_end, &l.a.next7, &l.a.prev, &l.a.active, &l.a.chosen, &l.a.grad,
	                  &l.a.gval, &l.a.cand6, &l.a.cand7, &l.a.values, &l.a.hpose, &l.a.hgrad, &l.a.hval, &l.a.end}) *f += shift;
	l.a.lin = l.lin; l.a.lm = l.lm; l.a.z = l.z;
	return l;
}

// room for `doubles` and the word read between rounds behind them; a reallocation waits for what the stream still holds
int multi_ensure(phd_navigator* nav, size_t doubles)
{
	if (nav->d_amulti && nav->h_amulti && doubles + 1 <= nav->amulti_cap) return PHD_OK;
	HC(hipStreamSynchronize(nav->stream));
	nav->amulti_cap = 0;
	HC(nav->d_amulti.alloc(doubles + 1));
	HC(nav->h_amulti.alloc(doubles + 1, hipHostMallocDefault));
	nav->amulti_cap = doubles + 1;
	return PHD_OK;
}

// The host's checks of a problem table, before anything is enqueued: the kernels index the pools with what passes here. zb: the
// block class of the call (1, 2, 4), 1 where no problem has a measurement.
int multi_validate(phd_navigator* nav, const char* who, int nproblems, const int32_t* lmoff, const double* landmarks3, const int32_t* zoff, const double* z3,
                   const int32_t* problem, int n, int* zb)
{
	const std::string w(who);
	if (nproblems < 1 || !lmoff || !zoff || !problem) return nav->fail(PHD_ERR_BAD_ARGUMENT, w + ": nproblems < 1 or a NULL array");
	if (lmoff[0] != 0 || zoff[0] != 0) return nav->fail(PHD_ERR_BAD_ARGUMENT, w + ": an offsets array does not start at 0");
	const int mmax = std::min(nav->prm.max_measurements, 256);
	int cls = 0;
	for (int q = 0; q < nproblems; q++) {
		const long long J = (long long) lmoff[q + 1] - lmoff[q], M = (long long) zoff[q + 1] - zoff[q];
		if (J < 0 || M < 0) return nav->fail(PHD_ERR_BAD_ARGUMENT, w + ": an offsets array decreases");
		if (J > nav->Jcap || M > mmax) {
			return nav->fail(PHD_ERR_BAD_ARGUMENT, w + ": a problem is out of range (landmarks <= min(1024, max_quantity rounded up to 64), measurements <= min(max_measurements, 256))");
		}
		if (M > 0) {
			const int c = zb_of((int) M);
			if (cls && c != cls) return nav->fail(PHD_ERR_BAD_ARGUMENT, w + ": the measurement counts of one call lie in one block class (0..64, 65..128 or 129..256)");
			cls = c;
		}
	}
	if ((lmoff[nproblems] && !landmarks3) || (zoff[nproblems] && !z3)) return nav->fail(PHD_ERR_BAD_ARGUMENT, w + ": a NULL pool");
	for (int e = 0; e < n; e++) {
		if (problem[e] < 0 || problem[e] >= nproblems) return nav->fail(PHD_ERR_BAD_ARGUMENT, w + ": a problem index outside [0, nproblems)");
	}
	if (!all_finite(landmarks3, (size_t) lmoff[nproblems] * 3) || !all_finite(z3, (size_t) zoff[nproblems] * 3)) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, w + ": non-finite input (NaN or infinity) is not accepted");
	}
	*zb = cls ? cls : 1;
	return PHD_OK;
}

// the table and the pools into the pinned mirror; the device's view of them
QuasiProblems multi_pack(double* h, double* d, const MultiLayout& l, int nproblems, const int32_t* lmoff, const double* landmarks3, const int32_t* zoff,
                         const double* z3, const int32_t* problem, int n)
{
	std::memcpy(h + l.lmoff, lmoff, (size_t) (nproblems + 1) * 4);
	std::memcpy(h + l.zoff, zoff, (size_t) (nproblems + 1) * 4);
	std::memcpy(h + l.problem, problem, (size_t) n * 4);
	if (lmoff[nproblems]) std::memcpy(h + l.lm, landmarks3, (size_t) lmoff[nproblems] * 3 * 8);
	if (zoff[nproblems]) std::memcpy(h + l.z, z3, (size_t) zoff[nproblems] * 3 * 8);
	QuasiProblems pr;
	pr.problem = (const int*) (d + l.problem); pr.lm_off = (const int*) (d + l.lmoff); pr.z_off = (const int*) (d + l.zoff);
	pr.lm = d + l.lm; pr.z = d + l.z; pr.lin = d + l.lin;
	return pr;
}

// an evaluation launch over many problems: M, z, qlm and qJ of `b` are bound per workgroup by the kernel
int multi_eval(phd_navigator* nav, const QuasiProblems& pr, int zb, int* flags, unsigned long long* slab, int average_mode, const double* poses7, int nposes,
               double* setll, double* qgrad, const int* active, int group)
{
	StepBufs b = make_bufs(nav);
	b.P = nposes; b.M = 0; b.z = pr.z;
	b.qposes = poses7; b.qlm = pr.lm; b.qJ = 0;
	b.setll = setll; b.qgrad = qgrad; b.qavg = average_mode;
	b.flags = flags; b.bigws_used = slab;
	const StepVariant& v = variant(zb * 64, false);
	hipLaunchKernelGGL(qgrad ? v.multi_grad : v.multi, dim3(nposes), dim3(256), (size_t) v.assoc_lds(nav->cutcap), nav->stream, nav->dp, b, nav->cutcap, pr, active, group);
	HC(hipGetLastError());
	return PHD_OK;
}

}  // namespace

int phd_quasi_ascent(phd_navigator* nav, const double* initial6, int nestimates, const double* linearpoint7,
                     const double* landmarks3, int nlandmarks, const double* z3, int nmeasurements,
                     int average_mode, int max_iterations, int round_iterations,
                     double* poses6, double* values, int32_t* iterations, double* hessians36)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);   // as the batch calls: the particle state is not touched
	const int n = nestimates, J = nlandmarks, M = nmeasurements;
	if (n < 1 || (long long) n * PHD_ASCENT_LINE > nav->Pcap || J < 0 || J > nav->Jcap || M < 0 || M > nav->prm.max_measurements || M > 256 ||
	    !initial6 || !linearpoint7 || !poses6 || !values || !iterations || (J && !landmarks3) || (M && !z3)) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_quasi_ascent: sizes out of range (16 x estimates <= max_particles, landmarks <= min(1024, max_quantity rounded up to 64), measurements <= max_measurements) or a NULL array");
	}
	if (average_mode < 0 || average_mode > 1 || max_iterations < 1 || round_iterations < 0) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_quasi_ascent: average_mode is not 0 / 1, max_iterations < 1 or round_iterations < 0");
	}
	FINITE_OR_FAIL(nav, initial6, (size_t) n * 6, "phd_quasi_ascent");
	FINITE_OR_FAIL(nav, linearpoint7, 7, "phd_quasi_ascent");
	FINITE_OR_FAIL(nav, landmarks3, (size_t) J * 3, "phd_quasi_ascent");
	FINITE_OR_FAIL(nav, z3, (size_t) M * 3, "phd_quasi_ascent");
	enter(nav);
	int rc = ascent_ensure(nav);
	if (rc) return rc;
	const AscentLayout l = ascent_layout(n, J, M);
	double* const d = nav->d_ascent;
	double* const h = nav->h_ascent;
	const AscentBufs s = ascent_bufs(d, l, n);
	std::memcpy(h + l.lin, linearpoint7, 7 * 8);
	if (J) std::memcpy(h + l.lm, landmarks3, (size_t) J * 3 * 8);
	if (M) std::memcpy(h + l.z, z3, (size_t) M * 3 * 8);
	std::memset(h + l.head, 0, 4 * 8);
	std::memcpy(h + l.pose6, initial6, (size_t) n * 6 * 8);
	HC(hipMemcpyAsync(d, h, l.loglike * 8, hipMemcpyHostToDevice, nav->stream));
	hipStream_t st = nav->stream;
	int* const word = (int*) (h + ascent_layout((size_t) (nav->Pcap / PHD_ASCENT_LINE), (size_t) nav->Jcap, 256).end);
	rc = ascent_chain(nav, s, max_iterations, round_iterations, hessians36 != nullptr, word,
	                  [&](const double* poses7, int nposes, double* setll, double* qgrad, const int* active, int group) {
		return ascent_eval(nav, s, l, J, M, average_mode, poses7, nposes, setll, qgrad, active, group);
	});
	if (rc) return rc;
	HC(hipMemcpyAsync(h + l.head, d + l.head, ((hessians36 ? l.out_end : l.hess) - l.head) * 8, hipMemcpyDeviceToHost, st));
	HC(hipStreamSynchronize(st));
	std::memcpy(poses6, h + l.pose6, (size_t) n * 6 * 8);
	std::memcpy(values, h + l.loglike, (size_t) n * 8);
	std::memcpy(iterations, h + l.iters, (size_t) n * 4);
	if (hessians36) std::memcpy(hessians36, h + l.hess, (size_t) n * 36 * 8);
	int flags = 0, nactive = 0;
	std::memcpy(&flags, h + l.head, 4);
	std::memcpy(&nactive, h + l.head + 2, 4);
	if (flags & PHD_FLAG_BIG_CLUSTER) {
		return nav->fail(PHD_ERR_ASSOCIATION, "phd_quasi_ascent: an association cluster exceeds the on-device solver");
	}
	if (nactive > 0) {
		return nav->fail(PHD_ERR_CAPACITY, "phd_quasi_ascent: estimates were still climbing after max_iterations iterations (their state at the bound is returned)");
	}
	return PHD_OK;
}

// phd_quasi_ascent for the estimates of many problems in the same launches: estimate e is searched against problem problem[e]
int phd_quasi_ascent_multi(phd_navigator* nav, int nproblems, const int32_t* landmark_offsets, const double* landmarks3,
                           const int32_t* measurement_offsets, const double* z3, const double* linearpoints7,
                           const double* initial6, const int32_t* problem, int nestimates,
                           int average_mode, int max_iterations, int round_iterations,
                           double* poses6, double* values, int32_t* iterations, double* hessians36)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);   // as the single call
	const char* who = "phd_quasi_ascent_multi";
	const int n = nestimates;
	if (n < 1 || (long long) n * PHD_ASCENT_LINE > nav->Pcap || !initial6 || !linearpoints7 || !poses6 || !values || !iterations) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_quasi_ascent_multi: 1 <= estimates, 16 x estimates <= max_particles, no NULL array");
	}
	if (average_mode < 0 || average_mode > 1 || max_iterations < 1 || round_iterations < 0) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_quasi_ascent_multi: average_mode is not 0 / 1, max_iterations < 1 or round_iterations < 0");
	}
	int zb = 1;
	int rc = multi_validate(nav, who, nproblems, landmark_offsets, landmarks3, measurement_offsets, z3, problem, n, &zb);
	if (rc) return rc;
	FINITE_OR_FAIL(nav, initial6, (size_t) n * 6, "phd_quasi_ascent_multi");
	FINITE_OR_FAIL(nav, linearpoints7, (size_t) nproblems * 7, "phd_quasi_ascent_multi");
	enter(nav);
	const MultiLayout l = multi_layout(nproblems, n, landmark_offsets[nproblems], measurement_offsets[nproblems], (size_t) nproblems * 7);
	rc = multi_ensure(nav, l.a.end);
	if (rc) return rc;
	double* const d = nav->d_amulti;
	double* const h = nav->h_amulti;
	const QuasiProblems pr = multi_pack(h, d, l, nproblems, landmark_offsets, landmarks3, measurement_offsets, z3, problem, n);
	AscentBufs s = ascent_bufs(d, l.a, n);
	s.problem = pr.problem;
	std::memcpy(h + l.lin, linearpoints7, (size_t) nproblems * 7 * 8);
	std::memset(h + l.head, 0, 4 * 8);
	std::memcpy(h + l.a.pose6, initial6, (size_t) n * 6 * 8);
	hipStream_t st = nav->stream;
	HC(hipMemcpyAsync(d, h, l.a.loglike * 8, hipMemcpyHostToDevice, st));
	int* const word = (int*) (h + nav->amulti_cap - 1);
	rc = ascent_chain(nav, s, max_iterations, round_iterations, hessians36 != nullptr, word,
	                  [&](const double* poses7, int nposes, double* setll, double* qgrad, const int* active, int group) {
		return multi_eval(nav, pr, zb, s.flags, s.slab, average_mode, poses7, nposes, setll, qgrad, active, group);
	});
	if (rc) return rc;
	HC(hipMemcpyAsync(h + l.head, d + l.head, ((hessians36 ? l.a.out_end : l.a.hess) - l.head) * 8, hipMemcpyDeviceToHost, st));
	HC(hipStreamSynchronize(st));
	std::memcpy(poses6, h + l.a.pose6, (size_t) n * 6 * 8);
	std::memcpy(values, h + l.a.loglike, (size_t) n * 8);
	std::memcpy(iterations, h + l.a.iters, (size_t) n * 4);
	if (hessians36) std::memcpy(hessians36, h + l.a.hess, (size_t) n * 36 * 8);
	int flags = 0, nactive = 0;
	std::memcpy(&flags, h + l.head, 4);
	std::memcpy(&nactive, h + l.head + 2, 4);
	if (flags & PHD_FLAG_BIG_CLUSTER) {
		return nav->fail(PHD_ERR_ASSOCIATION, "phd_quasi_ascent_multi: an association cluster exceeds the on-device solver");
	}
	if (nactive > 0) {
		return nav->fail(PHD_ERR_CAPACITY, "phd_quasi_ascent_multi: estimates were still climbing after max_iterations iterations (their state at the bound is returned)");
	}
	return PHD_OK;
}

// phd_quasi_set_loglik / phd_quasi_set_loglik_grad for poses of many problems in one launch: pose i is evaluated against problem[i]
int phd_quasi_set_loglik_multi(phd_navigator* nav, int nproblems, const int32_t* landmark_offsets, const double* landmarks3,
                               const int32_t* measurement_offsets, const double* z3, const double* poses7, const int32_t* problem, int nposes,
                               int average_mode, double* out, double* gradients6)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);
	const char* who = "phd_quasi_set_loglik_multi";
	const int n = nposes;
	if (n < 1 || n > nav->Pcap || !poses7 || !out || average_mode < 0 || average_mode > 1) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_quasi_set_loglik_multi: 1 <= poses <= max_particles, no NULL array, average_mode 0 / 1");
	}
	int zb = 1;
	int rc = multi_validate(nav, who, nproblems, landmark_offsets, landmarks3, measurement_offsets, z3, problem, n, &zb);
	if (rc) return rc;
	FINITE_OR_FAIL(nav, poses7, (size_t) n * 7, "phd_quasi_set_loglik_multi");
	enter(nav);
	const MultiLayout l = multi_layout(nproblems, n, landmark_offsets[nproblems], measurement_offsets[nproblems], (size_t) n * 7);
	const size_t oo = l.head + 4, og = oo + n, end = og + (gradients6 ? (size_t) n * 6 : 0);
	rc = multi_ensure(nav, end);
	if (rc) return rc;
	double* const d = nav->d_amulti;
	double* const h = nav->h_amulti;
	const QuasiProblems pr = multi_pack(h, d, l, nproblems, landmark_offsets, landmarks3, measurement_offsets, z3, problem, n);
	std::memcpy(h + l.lin, poses7, (size_t) n * 7 * 8);   // (the poses stand where an ascent has its linearisation poses)
	std::memset(h + l.head, 0, 4 * 8);
	hipStream_t st = nav->stream;
	HC(hipMemcpyAsync(d, h, oo * 8, hipMemcpyHostToDevice, st));
	rc = multi_eval(nav, pr, zb, (int*) (d + l.head), (unsigned long long*) (d + l.head + 1), gradients6 ? average_mode : 0, d + l.lin, n, d + oo, gradients6 ? d + og : nullptr, nullptr, 1);
	if (rc) return rc;
	HC(hipMemcpyAsync(h + l.head, d + l.head, (end - l.head) * 8, hipMemcpyDeviceToHost, st));
	HC(hipStreamSynchronize(st));
	std::memcpy(out, h + oo, (size_t) n * 8);
	if (gradients6) std::memcpy(gradients6, h + og, (size_t) n * 6 * 8);
	int flags = 0;
	std::memcpy(&flags, h + l.head, 4);
	if (flags & PHD_FLAG_BIG_CLUSTER) {
		return nav->fail(PHD_ERR_ASSOCIATION, "phd_quasi_set_loglik_multi: an association cluster exceeds the on-device solver");
	}
	return PHD_OK;
}

namespace {

// phd_quasi_guesses_multi, in doubles (the int arrays two to a double). What the call is given and what the count pass leaves:
//   lm_off[np + 1] | z_off[np + 1] | tile_first[np + 1] | landmarks[sum J][3] | z[sum M][3] | lin[np][7] | pose0[np][6] | far[7] | head[4]   <- ONE copy in
//   | guess_offsets[np + 1] | tile_count[ntiles] | tile_scan[ntiles + 1]
// head: the flag word and the slab counter of this call's evaluations, its own.
struct GuessLayout { size_t lmoff, zoff, tfirst, lm, z, lin, pose0, far7, head, goff, tcount, tscan, end; };

GuessLayout guess_layout(size_t np, size_t sumJ, size_t sumM, size_t ntiles)
{
	GuessLayout l;
	l.lmoff = 0; l.zoff = l.lmoff + (np + 2) / 2; l.tfirst = l.zoff + (np + 2) / 2; l.lm = l.tfirst + (np + 2) / 2;
	l.z = l.lm + sumJ * 3; l.lin = l.z + sumM * 3; l.pose0 = l.lin + np * 7; l.far7 = l.pose0 + np * 6; l.head = l.far7 + 7;
	l.goff = l.head + 4; l.tcount = l.goff + (np + 2) / 2; l.tscan = l.tcount + (ntiles + 1) / 2; l.end = l.tscan + (ntiles + 2) / 2;
	return l;
}

// ... and per guess, for n guesses, once the total is known: the evaluated poses are the far pose of every problem, then the guesses
//   problem_of[np + n] | pairs[n][2] | guesses6[n][6] | poses7[np + n][7] | values[np + n]      (from pairs on: ONE copy out)
struct GuessOutLayout { size_t problem, pairs, guesses, poses, values, end; };

GuessOutLayout guess_out_layout(size_t np, size_t n)
{
	GuessOutLayout l;
	l.problem = 0; l.pairs = l.problem + (np + n + 1) / 2; l.guesses = l.pairs + n; l.poses = l.guesses + n * 6;
	l.values = l.poses + (np + n) * 7; l.end = l.values + np + n;
	return l;
}

int guess_ensure(phd_navigator* nav, DevBuf<double>& d, PinBuf<double>& h, size_t& cap, size_t doubles)
{
	if (d && h && doubles <= cap) return PHD_OK;
	HC(hipStreamSynchronize(nav->stream));
	cap = 0;
	HC(d.alloc(doubles));
	HC(h.alloc(doubles, hipHostMallocDefault));
	cap = doubles;
	return PHD_OK;
}

}  // namespace

// The guess loop of GuidedFitMixture for many problems, and the first evaluation of every guess (phd_guesses.h)
int phd_quasi_guesses_multi(phd_navigator* nav, int nproblems, const int32_t* landmark_offsets, const double* landmarks3,
                            const int32_t* measurement_offsets, const double* z3, const double* linearpoints7, const double* pose0s6,
                            const double* farpose7, double radius, int capacity, int32_t* guess_offsets, int32_t* pairs2,
                            double* guesses6, double* poses7, double* values, double* emptyspace)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);   // as the other multi calls
	const char* who = "phd_quasi_guesses_multi";
	if (!linearpoints7 || !pose0s6 || !farpose7 || !guess_offsets || !pairs2 || !guesses6 || !poses7 || !values || !emptyspace) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_quasi_guesses_multi: a NULL array");
	}
	if (!std::isfinite(radius) || !(radius > 0)) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_quasi_guesses_multi: the radius is not a positive finite number");
	int zb = 1;
	int rc = multi_validate(nav, who, nproblems, landmark_offsets, landmarks3, measurement_offsets, z3, landmark_offsets /* (no item names a problem) */, 0, &zb);
	if (rc) return rc;
	const int np = nproblems;
	if (capacity < np) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_quasi_guesses_multi: the capacity is below one guess (pose0) per problem");
	FINITE_OR_FAIL(nav, linearpoints7, (size_t) np * 7, "phd_quasi_guesses_multi");
	FINITE_OR_FAIL(nav, pose0s6, (size_t) np * 6, "phd_quasi_guesses_multi");
	FINITE_OR_FAIL(nav, farpose7, 7, "phd_quasi_guesses_multi");
	std::vector<int32_t> tfirst((size_t) np + 1, 0);
	long long most = (long long) np;   // guesses at most: every pair and a pose0 per problem
	int maxt = 1;
	for (int q = 0; q < np; q++) {
		const long long pairs = (long long) (landmark_offsets[q + 1] - landmark_offsets[q]) * (measurement_offsets[q + 1] - measurement_offsets[q]);
		const long long t = (pairs + PHD_GUESS_TILE - 1) / PHD_GUESS_TILE;
		most += pairs;
		if (most > 0x7fffffffLL || (long long) tfirst[q] + t > 0x7fffffffLL) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_quasi_guesses_multi: more pairs than a 32-bit guess offset counts");
		tfirst[q + 1] = tfirst[q] + (int32_t) t;
		maxt = std::max(maxt, (int) t);
	}
	const int ntiles = tfirst[np];
	enter(nav);
	const size_t sumJ = landmark_offsets[np], sumM = measurement_offsets[np];
	const GuessLayout l = guess_layout(np, sumJ, sumM, ntiles);
	rc = guess_ensure(nav, nav->d_guess, nav->h_guess, nav->guess_cap, l.end);
	if (rc) return rc;
	double* const d = nav->d_guess;
	double* const h = nav->h_guess;
	std::memcpy(h + l.lmoff, landmark_offsets, (size_t) (np + 1) * 4);
	std::memcpy(h + l.zoff, measurement_offsets, (size_t) (np + 1) * 4);
	std::memcpy(h + l.tfirst, tfirst.data(), (size_t) (np + 1) * 4);
	if (sumJ) std::memcpy(h + l.lm, landmarks3, sumJ * 3 * 8);
	if (sumM) std::memcpy(h + l.z, z3, sumM * 3 * 8);
	std::memcpy(h + l.lin, linearpoints7, (size_t) np * 7 * 8);
	std::memcpy(h + l.pose0, pose0s6, (size_t) np * 6 * 8);
	std::memcpy(h + l.far7, farpose7, 7 * 8);
	std::memset(h + l.head, 0, 4 * 8);
	hipStream_t st = nav->stream;
	HC(hipMemcpyAsync(d, h, l.goff * 8, hipMemcpyHostToDevice, st));
	GuessBufs g;
	g.np = np; g.ntiles = ntiles; g.capacity = 0;
	g.focal = nav->dp.focal; g.radius2 = radius * radius;
	g.lm_off = (const int*) (d + l.lmoff); g.z_off = (const int*) (d + l.zoff); g.tile_first = (const int*) (d + l.tfirst);
	g.lm = d + l.lm; g.z = d + l.z; g.lin = d + l.lin; g.pose0 = d + l.pose0; g.far7 = d + l.far7;
	g.tile_count = (int*) (d + l.tcount); g.tile_scan = (int*) (d + l.tscan); g.goff = (int*) (d + l.goff);
	g.problem_of = nullptr; g.poses7 = nullptr; g.pairs2 = nullptr; g.guesses6 = nullptr;
	const dim3 grid((unsigned) np, (unsigned) maxt);
	if (ntiles) hipLaunchKernelGGL(k_guess_count, grid, dim3(256), 0, st, g);
	hipLaunchKernelGGL(k_guess_offsets, dim3(1), dim3(256), 0, st, g);
	HC(hipGetLastError());
	HC(hipMemcpyAsync(h + l.goff, d + l.goff, (size_t) (np + 1) * 4, hipMemcpyDeviceToHost, st));
	HC(hipStreamSynchronize(st));
	const int32_t* const hoff = (const int32_t*) (h + l.goff);
	const long long n = hoff[np];
	if (n < np || n > most) return nav->fail(PHD_ERR_DEVICE, "phd_quasi_guesses_multi: the device counted an impossible number of guesses");
	std::memcpy(guess_offsets, hoff, (size_t) (np + 1) * 4);
	if (n > capacity) {
		return nav->fail(PHD_ERR_CAPACITY, "phd_quasi_guesses_multi: " + std::to_string(n) + " guesses, the output arrays hold " + std::to_string(capacity) + " (guess_offsets is set)");
	}
	const GuessOutLayout o = guess_out_layout(np, (size_t) n);
	rc = guess_ensure(nav, nav->d_gout, nav->h_gout, nav->gout_cap, o.end);
	if (rc) return rc;
	double* const dg = nav->d_gout;
	double* const hg = nav->h_gout;
	g.capacity = (int) n;
	g.problem_of = (int*) (dg + o.problem); g.pairs2 = (int*) (dg + o.pairs); g.guesses6 = dg + o.guesses; g.poses7 = dg + o.poses;
	hipLaunchKernelGGL(k_guess_emit, grid, dim3(256), 0, st, g);
	HC(hipGetLastError());
	// the first values: the far pose of every problem and every guess, at most max_particles poses a launch, back to back
	QuasiProblems pr;
	pr.lm_off = g.lm_off; pr.z_off = g.z_off; pr.lm = g.lm; pr.z = g.z; pr.lin = g.lin;
	int* const flags = (int*) (d + l.head);
	unsigned long long* const slab = (unsigned long long*) (d + l.head + 1);
	const long long all = (long long) np + n;
	for (long long s = 0; s < all; s += nav->Pcap) {
		const int count = (int) std::min<long long>(nav->Pcap, all - s);
		if (s) HC(hipMemsetAsync(slab, 0, 8, st));   // every launch finds the slab counter at zero, as a batch call's does
		pr.problem = g.problem_of + s;
		rc = multi_eval(nav, pr, zb, flags, slab, 0, g.poses7 + s * 7, count, dg + o.values + s, nullptr, nullptr, 1);
		if (rc) return rc;
	}
	HC(hipMemcpyAsync(hg + o.pairs, dg + o.pairs, (o.end - o.pairs) * 8, hipMemcpyDeviceToHost, st));
	HC(hipMemcpyAsync(h + l.head, d + l.head, 8, hipMemcpyDeviceToHost, st));
	HC(hipStreamSynchronize(st));
	int fl = 0;
	std::memcpy(&fl, h + l.head, 4);
	if (fl & PHD_FLAG_BIG_CLUSTER) {
		return nav->fail(PHD_ERR_ASSOCIATION, "phd_quasi_guesses_multi: an association cluster exceeds the on-device solver");
	}
	std::memcpy(pairs2, hg + o.pairs, (size_t) n * 8);
	std::memcpy(guesses6, hg + o.guesses, (size_t) n * 6 * 8);
	std::memcpy(poses7, hg + o.poses + (size_t) np * 7, (size_t) n * 7 * 8);
	std::memcpy(values, hg + o.values + np, (size_t) n * 8);
	std::memcpy(emptyspace, hg + o.values, (size_t) np * 8);
	return PHD_OK;
}

int phd_test_ascent_control(phd_navigator* nav, const double* pose6, const double* loglike, const double* gradients6, const double* values16,
                            int nestimates, const double* linearpoint7, double* cand6, double* cand7, int32_t* chosen,
                            double* newpose6, double* newloglike, double* nextpose7, int32_t* active)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);
	const int n = nestimates;
	if (n < 1 || (long long) n * PHD_ASCENT_LINE > nav->Pcap || !pose6 || !loglike || !gradients6 || !values16 || !linearpoint7 || !cand6 || !cand7 ||
	    !chosen || !newpose6 || !newloglike || !nextpose7 || !active) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_test_ascent_control: 16 x estimates <= max_particles, no NULL array");
	}
	enter(nav);
	int rc = ascent_ensure(nav);
	if (rc) return rc;
	const AscentLayout l = ascent_layout(n, 0, 0);
	double* const d = nav->d_ascent;
	const AscentBufs s = ascent_bufs(d, l, n);
	std::vector<double> head(4, 0.0);
	std::vector<int32_t> ones(n, 1), zeros(n, 0);
	std::vector<double> prev(n, -INFINITY);
	HC(hipStreamSynchronize(nav->stream));
	HC(hipMemcpy(d + l.lin, linearpoint7, 7 * 8, hipMemcpyHostToDevice));
	HC(hipMemcpy(d + l.head, head.data(), 4 * 8, hipMemcpyHostToDevice));
	HC(hipMemcpy(s.pose6, pose6, (size_t) n * 6 * 8, hipMemcpyHostToDevice));
	HC(hipMemcpy(s.loglike, loglike, (size_t) n * 8, hipMemcpyHostToDevice));
	HC(hipMemcpy(s.prev, prev.data(), (size_t) n * 8, hipMemcpyHostToDevice));
	HC(hipMemcpy(s.grad, gradients6, (size_t) n * 6 * 8, hipMemcpyHostToDevice));
	HC(hipMemcpy(s.active, ones.data(), (size_t) n * 4, hipMemcpyHostToDevice));
	HC(hipMemcpy(s.iterations, zeros.data(), (size_t) n * 4, hipMemcpyHostToDevice));
	HC(hipMemset(s.nextpose7, 0, (size_t) n * 7 * 8));
	hipLaunchKernelGGL(k_ascent_candidates, dim3(ascent_blocks(n * PHD_ASCENT_LINE)), dim3(256), 0, nav->stream, s);
	HC(hipGetLastError());
	HC(hipMemcpyAsync(s.values, values16, (size_t) n * PHD_ASCENT_LINE * 8, hipMemcpyHostToDevice, nav->stream));   // (no evaluation in between: the caller's values)
	hipLaunchKernelGGL(k_ascent_select, dim3(ascent_blocks(n)), dim3(256), 0, nav->stream, s);
	HC(hipGetLastError());
	HC(hipStreamSynchronize(nav->stream));
	HC(hipMemcpy(cand6, s.cand6, (size_t) n * PHD_ASCENT_LINE * 6 * 8, hipMemcpyDeviceToHost));
	HC(hipMemcpy(cand7, s.cand7, (size_t) n * PHD_ASCENT_LINE * 7 * 8, hipMemcpyDeviceToHost));
	HC(hipMemcpy(chosen, s.chosen, (size_t) n * 4, hipMemcpyDeviceToHost));
	HC(hipMemcpy(newpose6, s.pose6, (size_t) n * 6 * 8, hipMemcpyDeviceToHost));
	HC(hipMemcpy(newloglike, s.loglike, (size_t) n * 8, hipMemcpyDeviceToHost));
	HC(hipMemcpy(nextpose7, s.nextpose7, (size_t) n * 7 * 8, hipMemcpyDeviceToHost));
	HC(hipMemcpy(active, s.active, (size_t) n * 4, hipMemcpyDeviceToHost));
	return PHD_OK;
}

int phd_test_pairing(phd_navigator* nav, const double* matrix, int n, int mode, int modelsize, int maxcount,
                     int32_t* assignments, double* values, int* count)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);
	if (!matrix || !assignments || !values || !count || n < 1 || n > MURTY_NBIG || maxcount < 1 || (mode == 1 && n > 5) || mode < 0 || mode > 1) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_test_pairing: n in 1..256 (1..5 for the lexicographic order), mode 0 or 1, buffers for maxcount pairings");
	}
	enter(nav);
	HC(hipStreamSynchronize(nav->stream));
	DevBuf<double> dm, dv; DevBuf<int> da, dc; DevBuf<char> dbig;
	HC(dm.alloc((size_t) n * n));
	if (n > MURTY_NMAX) HC(dbig.alloc(murty_big_bytes(n)));
	HC(da.alloc((size_t) maxcount * n));
	HC(dv.alloc(maxcount));
	HC(dc.alloc(1));
	hipError_t e = hipMemcpy(dm, matrix, (size_t) n * n * 8, hipMemcpyHostToDevice);
	if (e == hipSuccess) {
		hipMemset(da, 0xff, (size_t) maxcount * n * 4);
		hipLaunchKernelGGL(k_test_pairing, dim3(1), dim3(64), 0, nav->stream, nav->d_murty, dbig, (const double*) dm, n, mode, modelsize, maxcount, da, dv, dc);
		e = hipStreamSynchronize(nav->stream);
	}
	int m = 0;
	if (e == hipSuccess) e = hipMemcpy(&m, dc, 4, hipMemcpyDeviceToHost);
	const int k = std::min(m, maxcount);
	if (e == hipSuccess && k > 0) e = hipMemcpy(assignments, da, (size_t) k * n * 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess && k > 0) e = hipMemcpy(values, dv, (size_t) k * 8, hipMemcpyDeviceToHost);
	if (e != hipSuccess) return nav->fail(PHD_ERR_DEVICE, std::string("phd_test_pairing: ") + hipGetErrorString(e));
	*count = m;
	return PHD_OK;
}

int phd_test_primitive(phd_navigator* nav, int op, const void* in, int64_t in_bytes, void* out, int64_t out_bytes)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);
	PrimLayout l;
	if (!primitive_layout(op, l)) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_test_primitive: unknown op");
	int64_t n = l.fixed_n;
	bool fits = in_bytes >= l.head && out && (in || in_bytes == 0);
	if (fits && !l.fixed_n) {
		n = (in_bytes - l.head) / l.in_rec;
		fits = n >= 1 && n <= PT_MAX_RECORDS && (in_bytes - l.head) == n * l.in_rec && (!l.whole || n % l.block == 0) && (op != PT_SMALL_DIV || n <= 1024);
	} else if (fits) {
		fits = in_bytes == l.head;
	}
	if (!fits || out_bytes != n * l.out_rec) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_test_primitive: the sizes do not match the op's record layout (phd_primitives_test.h)");
	}
	if (op == PT_SMALL_DIV) {
		for (int64_t t = 0; t < n; t++) {
			const int32_t d = ((const int32_t*) in)[t];
			if (d < 1 || d >= PT_SMALL_DIV_RANGE) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_test_primitive: small_div takes 1 <= d < 2^24");
		}
	}
	enter(nav);
	HC(hipStreamSynchronize(nav->stream));
	DevBuf<char> din, dout;
	HC(din.alloc((size_t) std::max<int64_t>(in_bytes, 8)));
	HC(dout.alloc((size_t) out_bytes));
	hipError_t e = in_bytes ? hipMemcpy(din, in, (size_t) in_bytes, hipMemcpyHostToDevice) : hipSuccess;
	if (e == hipSuccess) e = hipMemsetAsync(dout, 0, (size_t) out_bytes, nav->stream);   // (on the kernel's stream: it must land before the kernel writes)
	if (e == hipSuccess) {
		const dim3 grid = (op == PT_SMALL_DIV) ? dim3(PT_SMALL_DIV_RANGE / (256 * PT_SMALL_DIV_PER_THREAD), (unsigned) n) : dim3((unsigned) ((n + l.block - 1) / l.block));
		hipLaunchKernelGGL(k_test_primitive, grid, dim3(l.block), PT_LDS_DOUBLES * sizeof(double), nav->stream, op, (const char*) din, (char*) dout, (int) n);
		e = hipGetLastError();
		if (e == hipSuccess) e = hipStreamSynchronize(nav->stream);
	}
	if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t) out_bytes, hipMemcpyDeviceToHost);
	if (e != hipSuccess) return nav->fail(PHD_ERR_DEVICE, std::string("phd_test_primitive: ") + hipGetErrorString(e));
	return PHD_OK;
}

int phd_set_weights(phd_navigator* nav, const double* weights, int nparticles)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nparticles != nav->P || !weights) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_set_weights: particle count mismatch");
	FINITE_OR_FAIL(nav, weights, nparticles, "phd_set_weights");
	if (nav->multi) return multi_set_small(nav, nullptr, weights, nparticles);
	enter(nav);
	double* hs = stage_acquire(nav);
	std::memcpy(hs, weights, (size_t) nparticles * 8);
	HC(hipMemcpyAsync(nav->d_stage, hs, (size_t) nparticles * 8, hipMemcpyHostToDevice, nav->stream));
	stage_release(nav);
	StepBufs b = make_bufs(nav);
	hipLaunchKernelGGL(k_store_small, dim3((nparticles + 255) / 256), dim3(256), 0, nav->stream, b, (const double*) nullptr, (const double*) nav->d_stage, nparticles);
	HC(hipGetLastError());
	nav->stage_valid = false;
	return PHD_OK;
}

int phd_set_map(phd_navigator* nav, int particle, const double* w, const double* mean3, const double* cov9, int ncomp)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (ncomp < 0 || (ncomp > 0 && (!w || !mean3 || !cov9))) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_set_map: bad map arrays");
	FINITE_OR_FAIL(nav, w, ncomp, "phd_set_map");
	FINITE_OR_FAIL(nav, mean3, (size_t) ncomp * 3, "phd_set_map");
	FINITE_OR_FAIL(nav, cov9, (size_t) ncomp * 9, "phd_set_map");
	if (nav->multi) return multi_set_map(nav, particle, w, mean3, cov9, ncomp);
	if (particle < 0 || particle >= nav->P) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_set_map: particle out of range");
	enter(nav);
	int rc = sync_state(nav);
	if (rc) return rc;
	rc = materialise(nav);   // a particle's slot may be shared with the other copies of its resampling source
	if (rc) return rc;
	return upload_particle(nav, cur_bank(nav), particle, w, mean3, cov9, ncomp);
}

// bulk upload of the whole particle set in the device layout (bench / tests):
// planes[10][nparticles][stride] (w, mx, my, mz, xx, xy, xz, yy, yz, zz), counts[nparticles],
// poses[nparticles][7], weights[nparticles]. Sets the particle count.
// (plane_stride: doubles between two planes of the host array — a shard of a multi-device handle takes its rows of every plane)
static int upload_impl(phd_navigator* nav, int nparticles, int stride, const double* planes, size_t plane_stride, const int32_t* counts,
                       const double* poses7, const double* weights)
{
	if (nparticles < 1 || nparticles > nav->Pcap || stride < 0 || stride > nav->cap) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_upload_state_soa: sizes out of range");
	enter(nav);
	int rc = sync_state(nav);
	if (rc) return rc;
	rc = reset_indirection(nav);
	if (rc) return rc;
	int I = cur_bank(nav);
	if (stride > 0) {
		// the ABI's host layout is plane per field ([10][particles][stride], the round-1 device layout); the banks hold one
		// record per component: converted here, at the edge, in pieces of a few thousand particles
		const int chunk = std::max(1, (int) std::min<size_t>((size_t) nparticles, ((size_t) 64 << 20) / ((size_t) stride * MIX_REC * 8) + 1));
		std::vector<double> recs((size_t) chunk * stride * MIX_REC);
		for (int p0 = 0; p0 < nparticles; p0 += chunk) {
			const int np_ = std::min(chunk, nparticles - p0);
			for (int i = 0; i < np_; i++) {
				const int nc = std::min(std::max(counts[p0 + i], 0), stride);
				double* r = recs.data() + (size_t) i * stride * MIX_REC;
				for (int f = 0; f < MIX_REC; f++) {
					const double* src = planes + (size_t) f * plane_stride + (size_t) (p0 + i) * stride;
					for (int c = 0; c < nc; c++) r[(size_t) c * MIX_REC + f] = src[c];
				}
			}
			HC(hipMemcpy2D(nav->bank[I].mix + (size_t) p0 * nav->cap * MIX_REC, (size_t) nav->cap * MIX_REC * 8, recs.data(),
			               (size_t) stride * MIX_REC * 8, (size_t) stride * MIX_REC * 8, np_, hipMemcpyHostToDevice));
		}
	}
	HC(hipMemcpy(nav->bank[I].count, counts, (size_t) nparticles * 4, hipMemcpyHostToDevice));
	HC(hipMemcpy(nav->bank[I].poses, poses7, (size_t) nparticles * 7 * 8, hipMemcpyHostToDevice));
	HC(hipMemcpy(nav->bank[I].weights, weights, (size_t) nparticles * 8, hipMemcpyHostToDevice));
	nav->P = nparticles;
	nav->stage_valid = false;
	return logs_restart(nav);
}

int phd_upload_state_soa(phd_navigator* nav, int nparticles, int stride, const double* planes, const int32_t* counts,
                         const double* poses7, const double* weights)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nparticles < 1 || nparticles > nav->Pcap || stride < 0 || !counts || !poses7 || !weights || (stride > 0 && !planes)) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_upload_state_soa: sizes out of range");
	FINITE_OR_FAIL(nav, poses7, (size_t) nparticles * 7, "phd_upload_state_soa");
	FINITE_OR_FAIL(nav, weights, nparticles, "phd_upload_state_soa");
	for (int i = 0; i < nparticles; i++) {   // (the components a particle holds; what lies behind its count is not read)
		if (counts[i] < 0 || counts[i] > stride) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_upload_state_soa: a component count exceeds the stride");
		for (int f = 0; f < 10; f++) FINITE_OR_FAIL(nav, planes + ((size_t) f * nparticles + i) * stride, counts[i], "phd_upload_state_soa");
	}
	if (nav->multi) return multi_upload(nav, nparticles, stride, planes, counts, poses7, weights);
	return upload_impl(nav, nparticles, stride, planes, (size_t) nparticles * stride, counts, poses7, weights);
}

// bulk download in the same layout; planes must hold [10][P][stride] with stride >= the largest count
static int download_impl(phd_navigator* nav, int stride, double* planes, size_t plane_stride, int32_t* counts, double* poses7, double* weights)
{
	enter(nav);
	int rc = sync_state(nav);
	if (rc) return rc;
	if (stride < 0 || stride > nav->cap) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_download_state_soa: stride out of range");
	rc = materialise(nav);
	if (rc) return rc;
	int I = cur_bank(nav);
	HC(hipMemcpy(counts, nav->bank[I].count, (size_t) nav->P * 4, hipMemcpyDeviceToHost));
	if (stride > 0) {   // records -> the ABI's planes (see upload_impl); slots behind a particle's count are left as they are
		const int chunk = std::max(1, (int) std::min<size_t>((size_t) nav->P, ((size_t) 64 << 20) / ((size_t) stride * MIX_REC * 8) + 1));
		std::vector<double> recs((size_t) chunk * stride * MIX_REC);
		for (int p0 = 0; p0 < nav->P; p0 += chunk) {
			const int np_ = std::min(chunk, nav->P - p0);
			HC(hipMemcpy2D(recs.data(), (size_t) stride * MIX_REC * 8, nav->bank[I].mix + (size_t) p0 * nav->cap * MIX_REC,
			               (size_t) nav->cap * MIX_REC * 8, (size_t) stride * MIX_REC * 8, np_, hipMemcpyDeviceToHost));
			for (int i = 0; i < np_; i++) {
				const int nc = std::min(std::max(counts[p0 + i], 0), stride);
				const double* r = recs.data() + (size_t) i * stride * MIX_REC;
				for (int f = 0; f < MIX_REC; f++) {
					double* dst = planes + (size_t) f * plane_stride + (size_t) (p0 + i) * stride;
					for (int c = 0; c < nc; c++) dst[c] = r[(size_t) c * MIX_REC + f];
				}
			}
		}
	}
	if (poses7) HC(hipMemcpy(poses7, nav->bank[I].poses, (size_t) nav->P * 7 * 8, hipMemcpyDeviceToHost));
	if (weights) HC(hipMemcpy(weights, nav->bank[I].weights, (size_t) nav->P * 8, hipMemcpyDeviceToHost));
	return PHD_OK;
}

int phd_download_state_soa(phd_navigator* nav, int stride, double* planes, int32_t* counts, double* poses7, double* weights)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) return multi_download(nav, stride, planes, counts, poses7, weights);
	return download_impl(nav, stride, planes, (size_t) nav->P * stride, counts, poses7, weights);
}

int phd_set_measurements(phd_navigator* nav, const double* z3, int nmeasurements)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nmeasurements < 0 || nmeasurements > nav->prm.max_measurements || (nmeasurements > 0 && !z3)) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_set_measurements: count out of range");
	FINITE_OR_FAIL(nav, z3, (size_t) nmeasurements * 3, "phd_set_measurements");
	if (nav->multi) return multi_set_measurements(nav, z3, nmeasurements);
	enter(nav);
	if (nmeasurements > 0) {
		double* hs = stage_acquire(nav);
		std::memcpy(hs, z3, (size_t) nmeasurements * 3 * 8);
		HC(hipMemcpyAsync(nav->d_z, hs, (size_t) nmeasurements * 3 * 8, hipMemcpyHostToDevice, nav->stream));
		stage_release(nav);
	}
	nav->M = nmeasurements;
	return PHD_OK;
}

// The depth map of the Kinect model. Validated in full before anything changes; a (re)allocation waits for the handle's
// streams (the kernels of posted steps may still read the old buffer) and the new buffers exist before the old ones go, so that a
// failed allocation leaves the previous map in place. Otherwise asynchronous: the frame goes through a pinned slot (whose previous copy
// has finished: its event) into the device buffer on the handle's stream, behind every kernel of the steps posted before (the
// stream the next step forks from is ordered behind all of them, phd_step_async) and before those of the next.
int phd_set_depth_map(phd_navigator* nav, const float* depth, int width, int height)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->prm.model != PHD_MODEL_PRM3D) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_set_depth_map: the depth map belongs to the PRM3D model (KinectMeasurer)");
	const bool off = !depth && width == 0 && height == 0;
	if (!off && (!depth || width < 1 || width > PHD_DEPTH_MAX || height < 1 || height > PHD_DEPTH_MAX)) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_set_depth_map: width and height in 1..4096 with a buffer, or NULL with 0 x 0 (no map)");
	}
	if (nav->multi) return multi_set_depth_map(nav, depth, width, height);
	enter(nav);
	if (off) {
		nav->dp.depth = nullptr; nav->dp.depth_w = 0; nav->dp.depth_h = 0; nav->dp.depth_hx = 0; nav->dp.depth_hy = 0;
		return PHD_OK;
	}
	const size_t n = (size_t) width * height;
	if (n > nav->depthcap || n > nav->hdepthcap) {
		HC(hipStreamSynchronize(nav->stream));
		for (int s = 0; s < phd_navigator::MAXSPLIT - 1; s++) if (nav->aux[s]) HC(hipStreamSynchronize(nav->aux[s]));
		DevBuf<float> nd; PinBuf<float> nh[2];
		hipError_t e = nd.alloc(n);
		for (int i = 0; i < 2 && e == hipSuccess; i++) e = nh[i].alloc(n, hipHostMallocDefault);
		for (int i = 0; i < 2 && e == hipSuccess; i++) if (!nav->ev_depth[i]) e = hipEventCreateWithFlags(nav->ev_depth[i].put(), hipEventDisableTiming);
		if (e != hipSuccess) return nav->fail(PHD_ERR_DEVICE, std::string("phd_set_depth_map: allocation: ") + hipGetErrorString(e));
		nav->d_depth = std::move(nd); nav->depthcap = n;   // (the old buffers go here, behind the new ones)
		nav->h_depth[0] = std::move(nh[0]); nav->h_depth[1] = std::move(nh[1]); nav->hdepthcap = n;
		nav->depth_used[0] = nav->depth_used[1] = false;
	}
	nav->depth_i ^= 1;
	const int i = nav->depth_i;
	if (nav->depth_used[i]) HC(hipEventSynchronize(nav->ev_depth[i]));
	std::memcpy(nav->h_depth[i], depth, n * 4);
	HC(hipMemcpyAsync(nav->d_depth, nav->h_depth[i], n * 4, hipMemcpyHostToDevice, nav->stream));
	HC(hipEventRecord(nav->ev_depth[i], nav->stream));
	nav->depth_used[i] = true;
	nav->dp.depth = nav->d_depth; nav->dp.depth_w = width; nav->dp.depth_h = height;
	nav->dp.depth_hx = (double) ((float) width / 2.0f); nav->dp.depth_hy = (double) ((float) height / 2.0f);   // ResX / 2 (KinectMeasurer.cs:153)
	return PHD_OK;
}

int phd_test_detection_probability(phd_navigator* nav, const double* z3, int n, double* out)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);
	if (n < 0 || (n > 0 && (!z3 || !out))) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_test_detection_probability: n >= 0 points and both buffers");
	if (n == 0) return PHD_OK;
	enter(nav);
	DevBuf<double> dz, dout;
	HC(dz.alloc((size_t) n * 3));
	hipError_t e = dout.alloc(n);
	if (e == hipSuccess) e = hipMemcpyAsync(dz, z3, (size_t) n * 3 * 8, hipMemcpyHostToDevice, nav->stream);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(k_test_detection_probability, dim3((n + 255) / 256), dim3(256), 0, nav->stream, nav->dp, (const double*) dz, n, (double*) dout);
		e = hipGetLastError();
	}
	if (e == hipSuccess) e = hipMemcpyAsync(out, dout, (size_t) n * 8, hipMemcpyDeviceToHost, nav->stream);
	if (e == hipSuccess) e = hipStreamSynchronize(nav->stream);
	if (e != hipSuccess) return nav->fail(PHD_ERR_DEVICE, std::string("phd_test_detection_probability: ") + hipGetErrorString(e));
	return PHD_OK;
}

int phd_set_split(phd_navigator* nav, int nsplit)
{
	if (!nav || nsplit < 0 || nsplit > phd_navigator::MAXSPLIT) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) return multi_forward_int(nav, 0, nsplit);
	nav->nsplit = nsplit;
	return PHD_OK;
}

int phd_set_association_workspace(phd_navigator* nav, int64_t bytes)
{
	if (!nav || bytes < 0) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) return multi_forward_int(nav, 1, bytes);
	enter(nav);
	HC(hipStreamSynchronize(nav->stream));
	nav->d_bigws.reset();
	nav->bigws_bytes = 0;
	if (bytes > 0) {
		HC(nav->d_bigws.alloc((size_t) bytes));
		nav->bigws_bytes = (unsigned long long) bytes;
	}
	HC(hipMemset(nav->d_bigws_used, 0, 8));
	return PHD_OK;
}

int phd_set_frozen(phd_navigator* nav, uint8_t frozen)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) return multi_forward_int(nav, 2, frozen);
	nav->frozen = frozen != 0;
	return PHD_OK;
}

int phd_set_all_pairs(phd_navigator* nav, uint8_t all_pairs)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) return multi_forward_int(nav, 3, all_pairs);
	nav->all_pairs = all_pairs != 0;
	return PHD_OK;
}

int phd_step_async(phd_navigator* nav, uint8_t onlymapping, double u_resample)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) return multi_step(nav, onlymapping, u_resample);
	if (nav->P < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_step: no particles (call phd_reset first)");
	hipSetDevice(nav->device);   // (not enter(): a step behind a step leaves the streams ordered)
	nav->timing_now = (nav->timing_step++ % nav->timing_period) == 0;
	StepBufs b = make_bufs(nav);
	nav->d_res_slots = nav->d_src;
	// The step boundary with two sub-range streams. A fork before the step and a join behind it put two markers and a barrier
	// between the last k_alpha_density and k_normalise_resample, and one more between that and the next k_sweep: 22 + 21 us in
	// which the device runs nothing (scripts/timeline_step.py). Posted back to back, the steps need neither: the stream whose
	// chain starts second finishes last (`lagger`), k_normalise_resample goes behind ITS k_alpha_density (the other stream's
	// event is long recorded), its next k_sweep behind that — and so it leads the next step, the other stream, which waits for
	// the event, lags and takes the end of that one.
	const bool chain = nav->chain_ok[variant(nav->M, nav->dp.depth != nullptr).zi()] && nav->P <= nav->chain_max;
	const int want = nav->nsplit > 0 ? nav->nsplit : (nav->P >= 1024 ? 2 : 1);
	const bool pipe = nav->pipeline && !chain && want == 2 && nav->P >= 2 && nav->stream == nav->own_stream;
	int rc;
	if (pipe) {
		if (!nav->pipe_ok) {
			// something else was enqueued on the stream since the last step (or this is the first): fork, `stream` leads
			HC(hipEventRecord(nav->ev_fork, nav->stream));
			HC(hipStreamWaitEvent(nav->aux[0], nav->ev_fork, 0));
			nav->lagger = 1;
		}
		hipStream_t L = nav->lagger ? nav->aux[0] : nav->stream, X = nav->lagger ? nav->stream : nav->aux[0];
		rc = launch_map(nav, b, !onlymapping, nav->lagger);
		if (rc) { nav->pipe_ok = false; return rc; }
		HC(hipEventRecord(nav->ev_join[0], X));
		HC(hipStreamWaitEvent(L, nav->ev_join[0], 0));
		{
			Timed t(nav, T_NR, L);
			rc = launch_normalise(nav, b, nullptr, nav->P, u_resample, onlymapping ? -1 : 0, onlymapping ? 1 : 0, nav->d_src, nav->d_info,
			                      nav->d_sel + (nav->parity ^ 1) * SEL_STRIDE, L);
		}
		if (rc) { nav->pipe_ok = false; return rc; }
		if (nav->hist_cap > 0 && !nav->frozen) {
			rc = hist_compose(nav, L);
			if (rc) { nav->pipe_ok = false; return rc; }
		}
		HC(hipEventRecord(nav->ev_res, L));
		HC(hipStreamWaitEvent(X, nav->ev_res, 0));
		nav->lagger ^= 1;
		nav->pipe_ok = true;
	}
	else {
		nav->pipe_ok = false;
		rc = launch_map(nav, b, !onlymapping);
		if (rc) return rc;
		{
			Timed t(nav, T_NR, nav->stream);
			// the same launch hands the resampled particles their small arrays and rotates the bank roles (rotate_roles)
			rc = launch_normalise(nav, b, nullptr, nav->P, u_resample, onlymapping ? -1 : 0, onlymapping ? 1 : 0, nav->d_src, nav->d_info,
			                      nav->d_sel + (nav->parity ^ 1) * SEL_STRIDE);
		}
		if (rc) return rc;
		if (nav->hist_cap > 0 && !nav->frozen) {
			rc = hist_compose(nav, nav->stream);
			if (rc) return rc;
		}
	}
	nav->parity ^= 1;
	nav->stage_valid = false;
	nav->sel_host_valid = false;   // the rotation depends on the resampling flag, known only on the device
	return PHD_OK;
}

int phd_sync(phd_navigator* nav)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) return multi_sync(nav);
	enter(nav);
	int rc = sync_state(nav);
	if (rc) return rc;
	rc = check_flags(nav);
	if (nav->h_flags) {
		hipMemset(nav->d_flags, 0, 4);
	}
	if (!rc && nav->plan_on_device && nav->sharded_used) {
		// the host never saw the plan of the last sharded step: what it said (a flag on another rank drops the step here too)
		int st[2] = {MIG_OK, 0};
		static_assert(MC_RESAMPLED == MC_STATUS + 1, "read together");
		HC(hipMemcpy(st, nav->plan.counts + mig_word(nav->world, MC_STATUS), 8, hipMemcpyDeviceToHost));
		nav->h_info[1] = st[1];
		if (st[0] == MIG_DROPPED) rc = nav->fail(PHD_ERR_GENERIC, "the step was dropped: another rank raised a flag (its phd_sync says which); the state is the one before the step");
		else if (st[0] == MIG_BAD) rc = nav->fail(PHD_ERR_GENERIC, "the gathered source vector was not a resampling result (were the weights of all ranks gathered?)");
		else if (st[0] == MIG_OVERFLOW) rc = nav->fail(PHD_ERR_CAPACITY, "more migrating particles than the send list holds");
	}
	return rc;
}

int phd_slam_update(phd_navigator* nav, const double* z3, int nmeasurements, uint8_t onlymapping, double u_resample)
{
	int rc = phd_set_measurements(nav, z3, nmeasurements);
	if (rc) return rc;
	rc = phd_step_async(nav, onlymapping, u_resample);
	if (rc) return rc;
	return phd_sync(nav);
}

const double* phd_weights(phd_navigator* nav, int* length)
{
	if (!nav) return nullptr;
	if (nav->multi) return multi_weights(nav, length);
	enter(nav);
	if (sync_state(nav)) return nullptr;
	int bidx = res_small(nav);
	nav->h_weights.resize(std::max(nav->P, 1));
	if (hipMemcpy(nav->h_weights.data(), nav->bank[bidx].weights, (size_t) nav->P * 8, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
	if (length) *length = nav->P;
	return nav->h_weights.data();
}

int phd_best_particle(phd_navigator* nav)
{
	if (!nav) return -1;
	if (nav->multi) return multi_best_particle(nav);
	enter(nav);
	if (sync_state(nav)) return -1;
	return nav->h_info[0];
}

const double* phd_poses(phd_navigator* nav, int* length)
{
	if (!nav) return nullptr;
	if (nav->multi) return multi_poses(nav, length);
	enter(nav);
	if (sync_state(nav)) return nullptr;
	int bidx = res_small(nav);
	nav->h_poses.resize((size_t) std::max(nav->P, 1) * 7);
	if (hipMemcpy(nav->h_poses.data(), nav->bank[bidx].poses, (size_t) nav->P * 7 * 8, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
	if (length) *length = nav->P * 7;
	return nav->h_poses.data();
}

int phd_map(phd_navigator* nav, int particle, int* ncomp, const double** w, const double** mean3, const double** cov9)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) return multi_map(nav, particle, ncomp, w, mean3, cov9);
	if (particle < 0 || particle >= nav->P || !ncomp) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map: particle out of range");
	enter(nav);
	int rc = sync_state(nav);
	if (rc) return rc;
	rc = fetch_map(nav, res_small(nav), particle, ncomp, res_mix(nav), res_slots(nav));
	if (rc) return rc;
	if (w) *w = nav->h_mw.data();
	if (mean3) *mean3 = nav->h_mm.data();
	if (cov9) *cov9 = nav->h_mc.data();
	return PHD_OK;
}

const int32_t* phd_resample_sources(phd_navigator* nav, int* length, uint8_t* resampled)
{
	if (!nav) return nullptr;
	if (nav->multi) return multi_resample_sources(nav, length, resampled);
	enter(nav);
	if (sync_state(nav)) return nullptr;
	nav->h_src.resize(std::max(nav->P, 1));
	if (hipMemcpy(nav->h_src.data(), nav->d_src, (size_t) nav->P * 4, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
	if (length) *length = nav->P;
	if (resampled) *resampled = nav->h_info[1] ? 1 : 0;
	return nav->h_src.data();
}

// ---- the trajectory log (phd_history.h) ---------------------------------------------------------
int phd_history_enable(phd_navigator* nav, int capacity)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_history_enable");
	if (capacity < 0) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_history_enable: capacity is the number of entries, 0 switches the log off");
	if (nav->sharded_used) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_history_enable: this handle runs sharded steps (sharded ancestry is not kept)");
	enter(nav);
	// (kernels of posted steps may still write the buffers that go)
	HC(hipStreamSynchronize(nav->stream));
	for (int s = 0; s < phd_navigator::MAXSPLIT - 1; s++) if (nav->aux[s]) HC(hipStreamSynchronize(nav->aux[s]));
	nav->hist_cap = 0; nav->hist_len = 0; nav->h_htimes.clear(); nav->h_hmark.clear();
	nav->d_hpose.reset(); nav->d_hparent.reset(); nav->d_hdirty.reset(); nav->d_hpend.reset();
	if (capacity == 0) return PHD_OK;
	const size_t rows = (size_t) capacity * nav->Pcap;
	hipError_t e = nav->d_hpose.alloc(rows * 7);
	if (e == hipSuccess) e = nav->d_hparent.alloc(rows);
	if (e == hipSuccess) e = nav->d_hdirty.alloc(capacity);
	if (e == hipSuccess) e = nav->d_hpend.alloc(2 * (size_t) nav->Pcap + 2);
	if (e == hipSuccess) e = hipMemsetAsync(nav->d_hdirty, 0, (size_t) capacity * 4, nav->stream);
	if (e != hipSuccess) {
		(void) hipGetLastError();
		nav->d_hpose.reset(); nav->d_hparent.reset(); nav->d_hdirty.reset(); nav->d_hpend.reset();
		return nav->fail(PHD_ERR_DEVICE, std::string("phd_history_enable: ") + std::to_string(rows * 60) + " bytes for the log: " + hipGetErrorString(e));
	}
	nav->hist_cap = capacity;
	nav->hist_pp = 0;
	return hist_restart(nav);
}

int phd_history_append(phd_navigator* nav, double time)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_history_append");
	if (nav->hist_cap < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_history_append: the trajectory log is off (phd_history_enable)");
	if (nav->P < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_history_append: no particles (call phd_reset first)");
	if (nav->hist_len >= nav->hist_cap) return nav->fail(PHD_ERR_CAPACITY, "phd_history_append: the trajectory log is full (" + std::to_string(nav->hist_cap) + " entries)");
	enter(nav);
	const int k = nav->hist_len, o = nav->hist_pp, n = o ^ 1;
	const size_t row = (size_t) k * nav->Pcap;
	StepBufs b = make_bufs(nav);
	hipLaunchKernelGGL(k_hist_append, dim3((nav->P * 7 + 255) / 256), dim3(256), 0, nav->stream, b, nav->P, nav->d_hpose + row * 7, nav->d_hparent + row, nav->d_hdirty + k,
	                   (const int*) nav->hpend(o), (const int*) nav->hpdirty(o), nav->hpend(n), nav->hpdirty(n));
	HC(hipGetLastError());
	nav->hist_pp = n;
	nav->hist_len = k + 1;
	nav->h_htimes.push_back(time);
	if (k == 0) nav->hist_mepoch = nav->mlog_cap > 0 ? nav->mlog_epoch : -1;
	nav->h_hmark.push_back(nav->mlog_len);
	return PHD_OK;
}

// phd_trajectories (entry < 0: the particles of the current state, through the pending map) and phd_trajectories_at (the
// particles that held the slots at `entry`: the log's first entry + 1 rows, no pending map). `what`: how `who` calls its list.
static int trajectories(phd_navigator* nav, const char* who, const char* what, int entry, const int32_t* particles, int nparticles, int* length, const double** times,
                        const double** poses7, const int32_t** slots)
{
	if (nav->hist_cap < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, std::string(who) + ": the trajectory log is off (phd_history_enable)");
	if (!particles || nparticles < 1 || !length) return nav->fail(PHD_ERR_BAD_ARGUMENT, std::string(who) + ": a list of at least one " + what + " and `length`");
	if (entry >= nav->hist_len) return nav->fail(PHD_ERR_BAD_ARGUMENT, std::string(who) + ": entry " + std::to_string(entry) + " of " + std::to_string(nav->hist_len));
	for (int i = 0; i < nparticles; i++) {
		if (particles[i] < 0 || particles[i] >= nav->P) return nav->fail(PHD_ERR_BAD_ARGUMENT, std::string(who) + ": " + what + " " + std::to_string(particles[i]) + " out of range");
	}
	enter(nav);
	const int L = entry < 0 ? nav->hist_len : entry + 1;
	const size_t cells = std::max((size_t) nparticles * L, (size_t) 1);
	if ((size_t) nparticles > nav->tqcap) {
		nav->tqcap = 0;
		HC(nav->d_tq.alloc(nparticles));
		HC(nav->h_tq.alloc(nparticles, hipHostMallocDefault));
		nav->tqcap = nparticles;
	}
	if (cells > nav->tcap) {
		const size_t want = std::max(cells, nav->tcap + nav->tcap / 2);
		nav->tcap = 0;
		nav->d_tpose.reset(); nav->d_tslot.reset(); nav->h_tpose.reset(); nav->h_tslot.reset();   // (the old ones go first: the buffers can be large)
		HC(nav->d_tpose.alloc(want * 7));
		HC(nav->d_tslot.alloc(want));
		HC(nav->h_tpose.alloc(want * 7, hipHostMallocDefault));
		HC(nav->h_tslot.alloc(want, hipHostMallocDefault));
		nav->tcap = want;
	}
	if (L > 0) {
		std::memcpy(nav->h_tq, particles, (size_t) nparticles * 4);
		HC(hipMemcpyAsync(nav->d_tq, nav->h_tq, (size_t) nparticles * 4, hipMemcpyHostToDevice, nav->stream));
		const int o = nav->hist_pp;
		hipLaunchKernelGGL(k_hist_trace, dim3((nparticles + 3) / 4), dim3(256), 0, nav->stream, (const double*) nav->d_hpose, (const int*) nav->d_hparent, (const int*) nav->d_hdirty,
		                   entry < 0 ? (const int*) nav->hpend(o) : nullptr, (const int*) nav->hpdirty(o), (const int*) nav->d_tq, nparticles, L, nav->P, nav->Pcap,
		                   (double*) nav->d_tpose, (int*) nav->d_tslot);
		HC(hipGetLastError());
		HC(hipMemcpyAsync(nav->h_tpose, nav->d_tpose, (size_t) nparticles * L * 7 * 8, hipMemcpyDeviceToHost, nav->stream));
		HC(hipMemcpyAsync(nav->h_tslot, nav->d_tslot, (size_t) nparticles * L * 4, hipMemcpyDeviceToHost, nav->stream));
	}
	HC(hipStreamSynchronize(nav->stream));
	*length = L;
	if (times) *times = nav->h_htimes.data();
	if (poses7) *poses7 = nav->h_tpose;
	if (slots) *slots = nav->h_tslot;
	return PHD_OK;
}

int phd_trajectories(phd_navigator* nav, const int32_t* particles, int nparticles, int* length, const double** times, const double** poses7, const int32_t** slots)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_trajectories");
	return trajectories(nav, "phd_trajectories", "particle", -1, particles, nparticles, length, times, poses7, slots);
}

int phd_trajectories_at(phd_navigator* nav, int entry, const int32_t* slots, int nslots, int* length, const double** times, const double** poses7, const int32_t** out_slots)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_trajectories_at");
	if (entry < 0) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_trajectories_at: entry " + std::to_string(entry) + " (entries count from 0)");
	return trajectories(nav, "phd_trajectories_at", "slot", entry, slots, nslots, length, times, poses7, out_slots);
}

// ---- the map log (phd_maplog.h) -------------------------------------------------------------------
int phd_map_history_enable(phd_navigator* nav, int entries, int64_t components)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_map_history_enable");
	if (entries < 0 || components < 0) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_history_enable: entries and components are counts, entries = 0 switches the log off");
	if (nav->sharded_used) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_history_enable: this handle runs sharded steps (the best particle may live on another shard)");
	// (the byte count of the records must fit a size_t: the kernel's bound is `components`, the buffer must be that large)
	if ((uint64_t) components > SIZE_MAX / (MIX_REC * sizeof(double))) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_history_enable: components beyond what can be addressed");
	enter(nav);
	// (kernels of posted steps and appends may still write the buffers that go)
	HC(hipStreamSynchronize(nav->stream));
	for (int s = 0; s < phd_navigator::MAXSPLIT - 1; s++) if (nav->aux[s]) HC(hipStreamSynchronize(nav->aux[s]));
	nav->mlog_cap = 0; nav->mlog_len = 0; nav->mlog_comps = 0; nav->h_mltimes.clear();
	nav->mlog_epoch++;
	nav->d_mlrec.reset(); nav->d_mlentry.reset(); nav->d_mlbump.reset();
	if (entries == 0) return PHD_OK;
	hipError_t e = nav->d_mlrec.alloc((size_t) std::max<int64_t>(components, 1) * MIX_REC);
	if (e == hipSuccess) e = nav->d_mlentry.alloc(entries);
	if (e == hipSuccess) e = nav->d_mlbump.alloc(2);
	if (e != hipSuccess) {
		(void) hipGetLastError();
		nav->d_mlrec.reset(); nav->d_mlentry.reset(); nav->d_mlbump.reset();
		return nav->fail(PHD_ERR_DEVICE, std::string("phd_map_history_enable: ") + std::to_string((long long) components) + " components of 80 bytes and " + std::to_string(entries) +
		                 " entries for the log: " + hipGetErrorString(e));
	}
	nav->mlog_cap = entries;
	nav->mlog_comps = components;
	nav->mlog_pp = 0;
	return mlog_restart(nav);
}

int phd_map_history_append(phd_navigator* nav, double time)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_map_history_append");
	if (nav->mlog_cap < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_history_append: the map log is off (phd_map_history_enable)");
	if (nav->P < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_history_append: no particles (call phd_reset first)");
	if (nav->frozen) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_history_append: frozen mode (the best particle describes a result the state never took)");
	if (nav->mlog_len >= nav->mlog_cap) return nav->fail(PHD_ERR_CAPACITY, "phd_map_history_append: the map log is full (" + std::to_string(nav->mlog_cap) + " entries)");
	enter(nav);
	const int k = nav->mlog_len, o = nav->mlog_pp, n = o ^ 1;
	StepBufs b = make_bufs(nav);
	hipLaunchKernelGGL((k_maplog_append<MapLogEntry>), dim3((nav->cap * (MIX_REC / 2) + 255) / 256), dim3(256), 0, nav->stream, b, (const int*) nav->d_info, nav->P, nav->Pcap, (double*) nav->d_mlrec,
	                   (long long) nav->mlog_comps, nav->d_mlentry + k, (const long long*) (nav->d_mlbump + o), nav->d_mlbump + n);
	HC(hipGetLastError());
	nav->mlog_pp = n;
	nav->mlog_len = k + 1;
	nav->h_mltimes.push_back(time);
	return PHD_OK;
}

int phd_map_history(phd_navigator* nav, int* length, const double** times, const int32_t** best, const double** best_pose7, const int32_t** counts, const int64_t** offsets,
                    const double** w, const double** mean3, const double** cov9)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_map_history");
	if (nav->mlog_cap < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_history: the map log is off (phd_map_history_enable)");
	if (!length) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_history: `length`");
	enter(nav);
	const int L = nav->mlog_len;
	nav->h_mlentry.resize(std::max(L, 1));
	if (L > 0) HC(hipMemcpyAsync(nav->h_mlentry.data(), nav->d_mlentry, (size_t) L * sizeof(MapLogEntry), hipMemcpyDeviceToHost, nav->stream));
	HC(hipStreamSynchronize(nav->stream));
	nav->h_mlbest.resize(std::max(L, 1)); nav->h_mlcount.resize(std::max(L, 1)); nav->h_mloff.assign((size_t) L + 1, 0); nav->h_mlpose.resize((size_t) std::max(L, 1) * 7);
	int64_t used = 0;
	int firstbad = -1;
	for (int k = 0; k < L; k++) {
		const MapLogEntry& e = nav->h_mlentry[k];
		const int c = e.count;
		if (e.offset != used || c < -1 || c > nav->cap || used + std::max(c, 0) > nav->mlog_comps) return nav->fail(PHD_ERR_GENERIC, "phd_map_history: corrupt entry " + std::to_string(k));
		if (c < 0 && firstbad < 0) firstbad = k;
		nav->h_mlbest[k] = e.best; nav->h_mlcount[k] = c; nav->h_mloff[k] = used;
		std::memcpy(&nav->h_mlpose[(size_t) k * 7], e.pose, 7 * 8);
		used += std::max(c, 0);
	}
	nav->h_mloff[L] = used;
	const size_t n = (size_t) used;
	nav->h_mlrec.resize(std::max(n, (size_t) 1) * MIX_REC);
	if (n > 0) HC(hipMemcpy(nav->h_mlrec.data(), nav->d_mlrec, n * MIX_REC * 8, hipMemcpyDeviceToHost));
	nav->h_mlw.resize(std::max(n, (size_t) 1)); nav->h_mlm.resize(std::max(n, (size_t) 1) * 3); nav->h_mlc.resize(std::max(n, (size_t) 1) * 9);
	for (size_t c = 0; c < n; c++) unpack_record(nav->h_mlrec.data() + c * MIX_REC, &nav->h_mlw[c], &nav->h_mlm[c * 3], &nav->h_mlc[c * 9]);
	*length = L;
	if (times) *times = nav->h_mltimes.data();
	if (best) *best = nav->h_mlbest.data();
	if (best_pose7) *best_pose7 = nav->h_mlpose.data();
	if (counts) *counts = nav->h_mlcount.data();
	if (offsets) *offsets = nav->h_mloff.data();
	if (w) *w = nav->h_mlw.data();
	if (mean3) *mean3 = nav->h_mlm.data();
	if (cov9) *cov9 = nav->h_mlc.data();
	if (firstbad >= 0) return nav->fail(PHD_ERR_CAPACITY, "phd_map_history: entry " + std::to_string(firstbad) + " did not fit the log's " + std::to_string(nav->mlog_comps) +
	                                    " components and holds no records (count -1)");
	return PHD_OK;
}

// ---- the map error of every logged map (phd_maperror.h) --------------------------------------------
static_assert(PHD_MAP_ERROR_MAX == PHD_MAPERR_MAX, "include/phdhip.h states the bound the kernel's LDS plan gives");
int phd_map_error(phd_navigator* nav, const double* truth3, int ntruth, double cutoff, double order, const double* align_pose7, const uint8_t* has_reference,
                  int* length, const double** times, const double** ospa, const double** cardinality, const double** spatial, const int32_t** estimate_size)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_map_error");
	if (nav->mlog_cap < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_error: the map log is off (phd_map_history_enable)");
	if (!length) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_error: `length`");
	if (ntruth < 0 || ntruth > PHD_MAP_ERROR_MAX || (ntruth > 0 && !truth3))
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_error: " + std::to_string(ntruth) + " truth points (0 .. PHD_MAP_ERROR_MAX = " + std::to_string(PHD_MAP_ERROR_MAX) + ")");
	if (!(cutoff > 0) || !(order >= 1) || !std::isfinite(cutoff) || !std::isfinite(order)) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map_error: cutoff > 0 and order >= 1");
	const int L = nav->mlog_len;
	FINITE_OR_FAIL(nav, truth3, (size_t) ntruth * 3, "phd_map_error");
	if (align_pose7) FINITE_OR_FAIL(nav, align_pose7, (size_t) L * 14, "phd_map_error");
	enter(nav);
	if (L > nav->mecap || !nav->d_metruth) {
		const int want = std::max(L, std::max(nav->mecap * 2, 64));
		nav->mecap = 0;
		hipError_t e = nav->d_metruth.alloc((size_t) PHD_MAP_ERROR_MAX * 3);
		if (e == hipSuccess) e = nav->d_mealign.alloc((size_t) want * PHD_MAPERR_ALIGN);
		if (e == hipSuccess) e = nav->d_meout.alloc((size_t) want * 3);
		if (e == hipSuccess) e = nav->d_mesize.alloc((size_t) want + 1);
		if (e != hipSuccess) {
			(void) hipGetLastError();
			nav->d_metruth.reset(); nav->d_mealign.reset(); nav->d_meout.reset(); nav->d_mesize.reset();
			return nav->fail(PHD_ERR_DEVICE, std::string("phd_map_error: buffers for ") + std::to_string(want) + " entries: " + hipGetErrorString(e));
		}
		nav->mecap = want;
	}
	const int cap = nav->mecap, n1 = std::max(L, 1);
	nav->h_mealign.assign((size_t) n1 * PHD_MAPERR_ALIGN, 0.0);
	if (align_pose7) {
		for (int k = 0; k < L; k++) {
			if (has_reference && !has_reference[k]) continue;
			// (has | R[9] | c[3], the estimated location | dx[3]: phd_maperror.h)
			double* al = &nav->h_mealign[(size_t) k * PHD_MAPERR_ALIGN];
			const double* est7 = align_pose7 + (size_t) k * 14;
			al[0] = 1.0;
			monorfs::MapErrorAlignment(est7, est7 + 7, al + 1, al + 13);
			for (int i = 0; i < 3; i++) al[10 + i] = est7[i];
		}
	}
	nav->h_meout.assign((size_t) n1 * 3, 0.0); nav->h_mesize.assign((size_t) n1 + 1, 0);
	int flag = 0;
	if (L > 0) {
		// (pageable copies: the call waits for the device anyway, and the host arrays are free when each returns)
		if (ntruth > 0) HC(hipMemcpyAsync(nav->d_metruth, truth3, (size_t) ntruth * 3 * 8, hipMemcpyHostToDevice, nav->stream));
		HC(hipMemcpyAsync(nav->d_mealign, nav->h_mealign.data(), (size_t) L * PHD_MAPERR_ALIGN * 8, hipMemcpyHostToDevice, nav->stream));
		HC(hipMemsetAsync(nav->d_mesize + cap, 0, 4, nav->stream));
		hipLaunchKernelGGL((k_map_error<MapLogEntry>), dim3(L), dim3(256), 0, nav->stream, (const double*) nav->d_mlrec, (long long) nav->mlog_comps, nav->cap,
		                   (const MapLogEntry*) nav->d_mlentry, (const double*) nav->d_metruth, ntruth, cutoff, order, (const double*) nav->d_mealign,
		                   (double*) nav->d_meout, nav->d_meout + cap, nav->d_meout + 2 * (size_t) cap, (int*) nav->d_mesize, nav->d_mesize + cap);
		HC(hipGetLastError());
		for (int q = 0; q < 3; q++) HC(hipMemcpyAsync(&nav->h_meout[(size_t) q * L], nav->d_meout + (size_t) q * cap, (size_t) L * 8, hipMemcpyDeviceToHost, nav->stream));
		HC(hipMemcpyAsync(nav->h_mesize.data(), nav->d_mesize, (size_t) L * 4, hipMemcpyDeviceToHost, nav->stream));
		HC(hipMemcpyAsync(&flag, nav->d_mesize + cap, 4, hipMemcpyDeviceToHost, nav->stream));
	}
	HC(hipStreamSynchronize(nav->stream));
	*length = L;
	if (times) *times = nav->h_mltimes.data();
	if (ospa) *ospa = nav->h_meout.data();
	if (cardinality) *cardinality = nav->h_meout.data() + L;
	if (spatial) *spatial = nav->h_meout.data() + 2 * (size_t) L;
	if (estimate_size) *estimate_size = nav->h_mesize.data();
	if (flag) return nav->fail(PHD_ERR_GENERIC, "phd_map_error: the assignment of an entry met its bound (records in the log that are no numbers); its values are NaN");
	for (int k = 0; k < L; k++) {
		if (nav->h_mesize[k] < 0) return nav->fail(PHD_ERR_CAPACITY, "phd_map_error: entry " + std::to_string(k) + " did not fit the map log and holds no records (count -1); its values are NaN");
		if (nav->h_mesize[k] > PHD_MAP_ERROR_MAX)
			return nav->fail(PHD_ERR_CAPACITY, "phd_map_error: entry " + std::to_string(k) + " has an estimate of " + std::to_string(nav->h_mesize[k]) + " landmarks, more than PHD_MAP_ERROR_MAX = " +
			                 std::to_string(PHD_MAP_ERROR_MAX) + "; its values are NaN");
	}
	return PHD_OK;
}

// ---- the pose-error series over the trajectory log (phd_poseerror.h) -------------------------------
static_assert(PHD_POSE_ERROR_MAX == PHD_POSEERR_MAX, "include/phdhip.h states the bound the kernel's LDS plan gives");
int phd_pose_error(phd_navigator* nav, int mode, const double* truth7, int ntruth, const int32_t* slots, int first_entry, int ref_entry, double slam_time,
                   int* length, const double** times, const double** location, const double** rotation,
                   int* odo_length, const double** odo_times, const double** odo_location, const double** odo_rotation)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_pose_error");
	if (nav->hist_cap < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: the trajectory log is off (phd_history_enable)");
	const int L = nav->hist_len;
	if (L < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: the trajectory log is empty");
	if (!length || !odo_length) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: `length` and `odo_length`");
	if (mode < PHD_POSE_ERROR_TIMED || mode > PHD_POSE_ERROR_FILTER) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: mode " + std::to_string(mode) + " (0 timed, 1 smooth, 2 filter)");
	if (!truth7 || ntruth != L) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: " + std::to_string(ntruth) + " true poses for a log of " + std::to_string(L) + " entries (one per entry)");
	if (first_entry < 0 || first_entry >= L) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: first_entry " + std::to_string(first_entry) + " of " + std::to_string(L));
	if (ref_entry < 0) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: ref_entry " + std::to_string(ref_entry) + " (entries count from 0)");
	if (!std::isfinite(slam_time)) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: slam_time is not finite");
	FINITE_OR_FAIL(nav, truth7, (size_t) L * 7, "phd_pose_error");
	for (int k = 0; k < L; k++) {
		const double* q = truth7 + (size_t) k * 7 + 3;
		if (!(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3] > 0)) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: the true pose of entry " + std::to_string(k) + " has a quaternion of norm 0");
	}
	if (slots) {
		for (int k = 0; k < L; k++) {
			if (slots[k] < 0 || slots[k] >= nav->P) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: slot " + std::to_string(slots[k]) + " at entry " + std::to_string(k) + " out of range");
		}
	}
	else {
		if (nav->mlog_cap < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: slots == NULL needs the map log (phd_map_history_enable)");
		if (nav->hist_mepoch != nav->mlog_epoch)
			return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_pose_error: slots == NULL, and the map log was off or has been restarted since the trajectory log's first entry was made");
	}
	if (L > PHD_POSE_ERROR_MAX) return nav->fail(PHD_ERR_CAPACITY, "phd_pose_error: a log of " + std::to_string(L) + " entries, more than PHD_POSE_ERROR_MAX = " + std::to_string(PHD_POSE_ERROR_MAX));
	if (nav->P > PHD_POSEERR_MAX_PARTICLES) return nav->fail(PHD_ERR_CAPACITY, "phd_pose_error: " + std::to_string(nav->P) + " particles, more than the 65536 whose slots the kernel keeps in 16 bits");
	enter(nav);
	if (L > nav->pecap) {
		const int want = std::min(std::max(L, std::max(nav->pecap * 2, 64)), PHD_POSE_ERROR_MAX);
		nav->pecap = 0;
		hipError_t e = nav->d_petruth.alloc((size_t) want * 7);
		if (e == hipSuccess) e = nav->d_peout.alloc((size_t) want * 4);
		if (e == hipSuccess) e = nav->d_pesel.alloc(want);
		if (e == hipSuccess) e = nav->d_pestart.alloc(want);
		if (e != hipSuccess) {
			(void) hipGetLastError();
			nav->d_petruth.reset(); nav->d_peout.reset(); nav->d_pesel.reset(); nav->d_pestart.reset();
			return nav->fail(PHD_ERR_DEVICE, std::string("phd_pose_error: buffers for ") + std::to_string(want) + " entries: " + hipGetErrorString(e));
		}
		nav->pecap = want;
	}
	const int cap = nav->pecap;
	// the series' lengths and times: Timed one value per estimate; Smooth by entry; Filter by position behind first_entry
	const int base = mode == PHD_POSE_ERROR_SMOOTH ? 0 : first_entry;
	const int n = L - base;
	const int nodo = mode == PHD_POSE_ERROR_TIMED ? n : 1 + std::max(0, n - PHD_POSEERR_ODO);
	std::vector<double> t(nav->h_htimes.begin() + base, nav->h_htimes.end()), todo(nodo);
	for (int j = 0; j < nodo; j++) todo[j] = mode == PHD_POSE_ERROR_TIMED ? t[j] : t[j == 0 ? 0 : j + PHD_POSEERR_ODO - 1];
	// start_i of Timed mode: the estimates before i whose time lies before slam_time (Plot.cs:360-362)
	nav->h_pestart.assign(L, 0);
	for (int i = first_entry + 1; i < L; i++) nav->h_pestart[i] = nav->h_pestart[i - 1] + (nav->h_htimes[i - 1] < slam_time ? 1 : 0);
	if (slots) nav->h_pesel.assign(slots, slots + L);
	else nav->h_pesel = nav->h_hmark;
	std::vector<double> res((size_t) 2 * n + 2 * (size_t) nodo);
	// (pageable copies: the call waits for the device anyway, and the host arrays are free when each returns)
	HC(hipMemcpyAsync(nav->d_petruth, truth7, (size_t) L * 7 * 8, hipMemcpyHostToDevice, nav->stream));
	HC(hipMemcpyAsync(nav->d_pesel, nav->h_pesel.data(), (size_t) L * 4, hipMemcpyHostToDevice, nav->stream));
	HC(hipMemcpyAsync(nav->d_pestart, nav->h_pestart.data(), (size_t) L * 4, hipMemcpyHostToDevice, nav->stream));
	const size_t lds = ((size_t) L * sizeof(unsigned short) + 15) & ~(size_t) 15;   // the slot row: at most 48 KB
	hipLaunchKernelGGL((k_pose_error<MapLogEntry>), dim3(mode == PHD_POSE_ERROR_TIMED ? n : 1), dim3(256), lds, nav->stream, (const double*) nav->d_hpose, (const int*) nav->d_hparent,
	                   (const int*) nav->d_hdirty, L, nav->P, nav->Pcap, (const double*) nav->d_petruth, (const int*) nav->d_pesel, slots ? 0 : 1,
	                   (const MapLogEntry*) nav->d_mlentry, nav->mlog_len, (const int*) nav->d_pestart, mode, first_entry, ref_entry, (double*) nav->d_peout, cap);
	HC(hipGetLastError());
	for (int q = 0; q < 4; q++) {
		HC(hipMemcpyAsync(res.data() + (q < 2 ? (size_t) q * n : 2 * (size_t) n + (size_t) (q - 2) * nodo), nav->d_peout + (size_t) q * cap, (size_t) (q < 2 ? n : nodo) * 8,
		                  hipMemcpyDeviceToHost, nav->stream));
	}
	HC(hipStreamSynchronize(nav->stream));
	nav->h_peout.swap(res); nav->h_petimes.swap(t); nav->h_peodotimes.swap(todo);
	*length = n;
	*odo_length = nodo;
	if (times) *times = nav->h_petimes.data();
	if (location) *location = nav->h_peout.data();
	if (rotation) *rotation = nav->h_peout.data() + n;
	if (odo_times) *odo_times = nav->h_peodotimes.data();
	if (odo_location) *odo_location = nav->h_peout.data() + 2 * (size_t) n;
	if (odo_rotation) *odo_rotation = nav->h_peout.data() + 2 * (size_t) n + nodo;
	return PHD_OK;
}

// ---- stage-level entry points ------------------------------------------------------------------
int phd_stage_run(phd_navigator* nav, const double* z3, int nmeasurements, uint8_t with_alpha)
{
	MULTI_UNSUPPORTED(nav, "phd_stage_run");
	int rc = phd_set_measurements(nav, z3, nmeasurements);
	if (rc) return rc;
	if (nav->P < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_stage_run: no particles");
	rc = sync_state(nav);
	if (rc) return rc;
	StepBufs b = make_bufs(nav);
	b.emit_all = 1;   // PHD_STAGE_CORRECTED is the whole list down to MinWeight: no cut floor (phd_correct.h)
	HC(hipMemsetAsync(nav->d_bigws_used, 0, 8, nav->stream));
	rc = launch_map(nav, b, with_alpha != 0);
	if (rc) return rc;
	hipLaunchKernelGGL(k_expand_emit, dim3(nav->P), dim3(256), 0, nav->stream, nav->dp, b);   // PHD_STAGE_CORRECTED reads whole records
	HC(hipGetLastError());
	HC(hipMemsetAsync(nav->d_bigws_used, 0, 8, nav->stream));   // (as behind a quasi batch: no k_normalise_resample follows a stage run)
	rc = sync_state(nav);
	if (rc) return rc;
	nav->stage_valid = true;
	rc = check_flags(nav);
	if (nav->h_flags) hipMemset(nav->d_flags, 0, 4);
	return rc;
}

int phd_stage_map(phd_navigator* nav, int stage, int particle, int* ncomp, const double** w, const double** mean3,
                  const double** cov9)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_stage_map");
	if (!nav->stage_valid) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_stage_map: call phd_stage_run first");
	if (particle < 0 || particle >= nav->P || !ncomp) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_stage_map: particle out of range");
	enter(nav);
	int rc = PHD_OK;
	if (stage == PHD_STAGE_PRUNED) {
		rc = fetch_map(nav, nav->h_sel[SEL_OUT], particle, ncomp);
	}
	else if (stage == PHD_STAGE_PREDICTED) {
		int n = 0;
		rc = fetch_map(nav, nav->h_sel[SEL_IN], particle, &n, nav->h_sel[SEL_INMIX], nav->d_inslot);
		if (rc) return rc;
		int nb = 0;
		HC(hipMemcpy(&nb, nav->d_born_count + particle, 4, hipMemcpyDeviceToHost));
		std::vector<double> bm((size_t) std::max(nb, 1) * 3);
		if (nb > 0) HC(hipMemcpy(bm.data(), nav->d_born_mean + (size_t) particle * nav->Mcap * 3, (size_t) nb * 3 * 8, hipMemcpyDeviceToHost));
		nav->h_mw.resize(n + nb); nav->h_mm.resize((size_t) (n + nb) * 3); nav->h_mc.resize((size_t) (n + nb) * 9);
		for (int i = 0; i < nb; i++) {
			nav->h_mw[n + i] = nav->prm.birth_weight;
			for (int k = 0; k < 3; k++) nav->h_mm[(size_t) (n + i) * 3 + k] = bm[i * 3 + k];
			for (int k = 0; k < 9; k++) nav->h_mc[(size_t) (n + i) * 9 + k] = nav->prm.birth_covariance[k];
		}
		*ncomp = n + nb;
	}
	else if (stage == PHD_STAGE_CORRECTED) {
		int ne = 0;
		HC(hipMemcpy(&ne, nav->d_emit_count + particle, 4, hipMemcpyDeviceToHost));
		size_t eb = (size_t) particle * nav->ecap;
		std::vector<double> rec((size_t) std::max(ne, 1) * MIX_REC);
		nav->h_mw.resize(std::max(ne, 1)); nav->h_mm.resize((size_t) std::max(ne, 1) * 3); nav->h_mc.resize((size_t) std::max(ne, 1) * 9);
		if (ne > 0) {
			HC(hipMemcpy(nav->h_mw.data(), nav->d_emit_w + eb, (size_t) ne * 8, hipMemcpyDeviceToHost));
			HC(hipMemcpy(rec.data(), nav->d_emit_rec + eb * MIX_REC, (size_t) ne * MIX_REC * 8, hipMemcpyDeviceToHost));
		}
		for (int c = 0; c < ne; c++) {
			const double* r = &rec[(size_t) c * MIX_REC + 1];   // (mean and covariance behind the record's weight)
			for (int k = 0; k < 3; k++) nav->h_mm[(size_t) c * 3 + k] = r[k];
			double* C = &nav->h_mc[(size_t) c * 9];
			C[0] = r[3]; C[1] = r[4]; C[2] = r[5]; C[3] = r[4]; C[4] = r[6]; C[5] = r[7]; C[6] = r[5]; C[7] = r[7]; C[8] = r[8];
		}
		*ncomp = ne;
	}
	else {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_stage_map: unknown stage");
	}
	if (rc) return rc;
	if (w) *w = nav->h_mw.data();
	if (mean3) *mean3 = nav->h_mm.data();
	if (cov9) *cov9 = nav->h_mc.data();
	return PHD_OK;
}

const double* phd_stage_alpha(phd_navigator* nav, int* length)
{
	if (!nav || !nav->stage_valid) return nullptr;
	nav->h_alpha.resize(std::max(nav->P, 1));
	if (hipMemcpy(nav->h_alpha.data(), nav->d_alpha, (size_t) nav->P * 8, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
	if (length) *length = nav->P;
	return nav->h_alpha.data();
}

const double* phd_stage_setloglik(phd_navigator* nav, int* length)
{
	if (!nav || !nav->stage_valid) return nullptr;
	nav->h_setll.resize(std::max(nav->P, 1));
	if (hipMemcpy(nav->h_setll.data(), nav->d_setll, (size_t) nav->P * 8, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
	if (length) *length = nav->P;
	return nav->h_setll.data();
}

// the gathered weight vector of all ranks (+ room for their status words behind it) and the global source vector
static int ensure_gw(phd_navigator* nav, int n, bool shared = false)
{
	if (n <= nav->gwcap) return PHD_OK;
	if (nav->gw_shared) return nav->fail(PHD_ERR_GENERIC, "the gathered-weight vector of a shard cannot grow (other shards hold its address)");
	HC(hipStreamSynchronize(nav->stream));
	nav->d_gw.reset();
	nav->d_plan.reset();
	// (a multi-device handle's shards store their weights into each other's vectors: fine-grained, as the receive buffers)
	if (!shared || getenv("PHD_COARSE_RECV") || hipExtMallocWithFlags((void**) nav->d_gw.put(), ((size_t) n + PHD_MAX_DEVICES) * 8, hipDeviceMallocFinegrained) != hipSuccess) {
		(void) hipGetLastError();
		(void) nav->d_gw.release();   // (whatever the failed call left in it is nothing to free)
		HC(nav->d_gw.alloc((size_t) n + PHD_MAX_DEVICES));
	}
	HC(nav->d_plan.alloc(n));
	nav->gwcap = n;
	return PHD_OK;
}

int phd_resample(phd_navigator* nav, const double* weights, int nparticles, double u_resample, int32_t* sources,
                 int32_t* best_particle)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);
	if (nparticles < 1 || !weights || !sources) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_resample: bad arguments");
	enter(nav);
	HC(hipStreamSynchronize(nav->stream));
	// (buffers of its own: the gathered-weight vector of a sharded handle is known to other shards by address)
	DevBuf<double> d_w;
	DevBuf<int> d_src2;
	HC(d_w.alloc(nparticles));
	if (d_src2.alloc((size_t) nparticles + 2) != hipSuccess) return nav->fail(PHD_ERR_DEVICE, "phd_resample: out of device memory");
	hipError_t e = hipMemcpy(d_w, weights, (size_t) nparticles * 8, hipMemcpyHostToDevice);
	StepBufs b = make_bufs(nav);
	int rc = (e == hipSuccess) ? launch_normalise(nav, b, d_w, nparticles, u_resample, 1, 1, d_src2 + 2, d_src2) : PHD_OK;
	if (e == hipSuccess) e = hipStreamSynchronize(nav->stream);
	int info[2] = {0, 0};
	if (e == hipSuccess) e = hipMemcpy(sources, d_src2 + 2, (size_t) nparticles * 4, hipMemcpyDeviceToHost);
	if (e == hipSuccess) e = hipMemcpy(info, d_src2, 8, hipMemcpyDeviceToHost);
	if (rc) return rc;
	if (e != hipSuccess) return nav->fail(PHD_ERR_DEVICE, hipGetErrorString(e));
	if (best_particle) *best_particle = info[0];
	return PHD_OK;
}

int phd_particle_depleted(phd_navigator* nav, const double* weights, int nparticles, uint8_t* depleted)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);
	if (nparticles < 1 || !weights || !depleted) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_particle_depleted: bad arguments");
	enter(nav);
	HC(hipStreamSynchronize(nav->stream));
	DevBuf<double> d_w;
	DevBuf<int> d_tmp;
	HC(d_w.alloc(nparticles));
	if (d_tmp.alloc((size_t) nparticles + 2) != hipSuccess) return nav->fail(PHD_ERR_DEVICE, "phd_particle_depleted: out of device memory");
	hipError_t e = hipMemcpy(d_w, weights, (size_t) nparticles * 8, hipMemcpyHostToDevice);
	StepBufs b = make_bufs(nav);
	int rc = (e == hipSuccess) ? launch_normalise(nav, b, d_w, nparticles, 0.5, 0, 1, d_tmp + 2, d_tmp) : PHD_OK;
	if (e == hipSuccess) e = hipStreamSynchronize(nav->stream);
	int info[2] = {0, 0};
	if (e == hipSuccess) e = hipMemcpy(info, d_tmp, 8, hipMemcpyDeviceToHost);
	if (rc) return rc;
	if (e != hipSuccess) return nav->fail(PHD_ERR_DEVICE, hipGetErrorString(e));
	*depleted = info[1] ? 1 : 0;
	return PHD_OK;
}

#ifdef PHD_STAMPS
// diagnostic build only: per-workgroup phase stamps of the last stamped kernel, [P][16] doubles
int phd_debug_stamps(phd_navigator* nav, double* out)
{
	hipStreamSynchronize(nav->stream);
	return hipMemcpy(out, nav->d_stamps, (size_t) nav->P * 16 * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

void* phd_stream(phd_navigator* nav) { return (nav && !nav->multi) ? (void*) nav->stream : nullptr; }

int phd_timing_reset(phd_navigator* nav, uint8_t enabled)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) {   // the kernels of the first shard are the ones timed; the phases of its steps too (phd_multi_report)
		multi_timing_reset(nav, enabled);
		nav = multi_shard0(nav);
	}
	enter(nav);
	hipStreamSynchronize(nav->stream);
	nav->ntimers = 0;
	nav->timing = enabled != 0;
	nav->timing_period = enabled ? enabled : 1;   // 1: every step; n: every n-th step (sampling keeps the events' own cost small)
	nav->timing_step = 0;
	nav->timing_now = true;
	return PHD_OK;
}

int phd_last_timings(phd_navigator* nav, const char*** names, const double** ms)
{
	if (!nav) return 0;
	if (nav->multi) nav = multi_shard0(nav);
	enter(nav);
	hipStreamSynchronize(nav->stream);
	nav->tnames.clear();
	nav->tms.clear();
	nav->tcounts.clear();
	for (size_t r = 0; r < nav->ntimers; r++) {
		Timer& t = nav->timers[r];
		float f = 0;
		if (hipEventElapsedTime(&f, t.t0_from >= 0 ? nav->timers[t.t0_from].t1 : t.t0, t.t1) != hipSuccess) continue;
		size_t k = 0;
		for (; k < nav->tnames.size(); k++) {
			if (nav->tnames[k] == t.name) break;
		}
		if (k == nav->tnames.size()) { nav->tnames.push_back(t.name); nav->tms.push_back(0); nav->tcounts.push_back(0); }
		nav->tms[k] += (double) f;
		nav->tcounts[k]++;
	}
	for (size_t k = 0; k < nav->tms.size(); k++) nav->tms[k] /= std::max(nav->tcounts[k], 1);
	if (names) *names = nav->tnames.data();
	if (ms) *ms = nav->tms.data();
	return (int) nav->tnames.size();
}

int phd_last_timing_counts(phd_navigator* nav, const int** counts)
{
	if (!nav) return 0;
	if (nav->multi) nav = multi_shard0(nav);
	if (counts) *counts = nav->tcounts.data();
	return (int) nav->tcounts.size();
}

// ---- multi-GPU ----------------------------------------------------------------------------------
// Particles are sharded contiguously: rank r owns global slots [r * P, (r + 1) * P). One step is
//   phd_step_local_async                      predict / correct / prune / reweight of the shard; the weights are exported
//   <all-gather of phd_device_local_weights into phd_device_global_weights, RCCL, by the host>
//   phd_step_global_async                     normalise + BestParticle + depletion test + systematic resampling over ALL
//                                             particles, identical on every rank; then the migration plan, ON THE DEVICE
//   phd_migration_plan                        the host learns the 2 n split sizes of the exchange (nothing else crosses)
//   phd_migration_pack_async, <all-to-all of the send/recv buffers>, phd_migration_unpack_async
// A phd_create_multi handle plays the same kernels from one worker thread per shard, with peer stores in place of the
// collectives and no host wait anywhere (phd_multi.inc).

// Buffers of the sharded step, made once (their addresses go into other shards' tables): export buffer, plan arrays, pinned
// counts, send / receive buffers. With non-decreasing sources a rank receives at most one record per slot and sends at
// most Pcap + world - 1 (a source particle goes to every rank its run of slots meets; runs of successive sources share at
// most one rank).
static void free_sharded(phd_navigator* nav)
{
	nav->d_lw.reset();
	nav->d_dst_tab.reset();
	nav->plan_code.reset(); nav->plan_fslot.reset(); nav->plan_sendlist.reset(); nav->plan_senddst.reset(); nav->plan_counts.reset();
	nav->plan = MigPlan{nullptr, nullptr, nullptr, nullptr, nullptr, 0};
	nav->h_counts.reset();
	nav->d_mslot.reset();
	nav->d_plang.reset();
	nav->d_send.reset();
	nav->d_recv.reset();
	nav->d_recv_tab.reset();
	nav->sharded_ready = false;
}

// ints of one set of the grid plan's accumulators: cnt [64][64] | used [Pcap / 32 + 1] | bad [1]
static size_t plan_grid_set_words(const phd_navigator* nav) { return (size_t) PHD_MAX_DEVICES * PHD_MAX_DEVICES + (size_t) (nav->Pcap + 31) / 32 + 2; }

static int ensure_sharded(phd_navigator* nav, bool need_send = true)
{
	if (nav->sharded_ready) {
		if (need_send && !nav->d_send) {   // (a handle first used without a send buffer: push-only hosts never need one)
			enter(nav);
			HC(nav->d_send.alloc((size_t) nav->sendrecs * mig_rec_doubles(nav->cap)));
		}
		return PHD_OK;
	}
	enter(nav);
	nav->plan.sendcap = nav->Pcap + PHD_MAX_DEVICES;
	nav->recvrecs = nav->Pcap;
	nav->sendrecs = nav->plan.sendcap;
	// (all or nothing: a failure frees what was made, so that the call can be repeated and nothing downstream ever sees a
	// half-made set — the flag below is what every user of these buffers asks)
	hipError_t e = hipSuccess;
	auto want = [&](hipError_t r) { if (e == hipSuccess) e = r; return e == hipSuccess; };
	want(nav->d_lw.alloc((size_t) nav->Pcap + 1));
	want(nav->d_dst_tab.alloc(PHD_MAX_DEVICES));
	double* const lw = nav->d_lw;   // (the table's first entry is the ADDRESS the export buffer has on the device)
	if (e == hipSuccess) want(hipMemcpy(nav->d_dst_tab, &lw, sizeof(double*), hipMemcpyHostToDevice));
	want(nav->d_recv_tab.alloc(PHD_MAX_DEVICES));
	want(nav->plan_code.alloc(nav->Pcap));
	want(nav->plan_fslot.alloc(nav->Pcap));
	want(nav->plan_sendlist.alloc(nav->plan.sendcap));
	want(nav->plan_senddst.alloc(nav->plan.sendcap));
	want(nav->plan_counts.alloc(MIG_COUNT_WORDS));
	nav->plan = MigPlan{nav->plan_code, nav->plan_fslot, nav->plan_sendlist, nav->plan_senddst, nav->plan_counts, nav->plan.sendcap};
	if (e == hipSuccess) want(hipMemset(nav->plan.counts, 0, MIG_COUNT_WORDS * 4));
	// (coherent: the plan kernel's system-scope stores must reach the polling host while the kernel runs, whatever the
	// runtime's default for mapped host memory is)
	want(nav->h_counts.alloc(MIG_COUNT_WORDS, hipHostMallocMapped | hipHostMallocCoherent));
	if (e == hipSuccess) std::memset(nav->h_counts, 0, MIG_COUNT_WORDS * 4);
	want(nav->d_mslot.alloc(nav->Pcap));
	{   // k_plan_count / k_plan_lists: [2 sets] (plan_grid_set_words) | wcg [1024] | lcg [Pcap / 64 + 1]
		const size_t words = 2 * plan_grid_set_words(nav) + 1024 + (size_t) nav->Pcap / 64 + 2;
		want(nav->d_plang.alloc(words));
		if (e == hipSuccess) want(hipMemset(nav->d_plang, 0, words * 4));
	}
	if (need_send) want(nav->d_send.alloc((size_t) nav->sendrecs * mig_rec_doubles(nav->cap)));   // (a shard of a multi-device handle packs straight into its peers' receive buffers)
	// The receive buffer is written by OTHER devices (peer stores of a multi-device handle's shards, or of other ranks'
	// processes through IPC) and read here: fine-grained device memory, coherent between agents without cache maintenance —
	// what RCCL allocates for its own peer-to-peer buffers. (See the head of phd_multi.inc for the visibility argument.)
	if (e == hipSuccess) {
		// (behind the records: the landing flags, one word per sending rank — k_post_landing)
		const size_t recv_bytes = mig_recv_doubles(nav->recvrecs, nav->cap) * 8;
		nav->recv_finegrained = getenv("PHD_COARSE_RECV") == nullptr &&
		                        hipExtMallocWithFlags((void**) nav->d_recv.put(), recv_bytes, hipDeviceMallocFinegrained) == hipSuccess;
		if (!nav->recv_finegrained) {
			(void) hipGetLastError();
			(void) nav->d_recv.release();   // (whatever the failed call left in it is nothing to free)
			want(nav->d_recv.alloc(recv_bytes / 8));
		}
		if (e == hipSuccess) want(hipMemset(nav->d_recv + mig_landing_offset(nav->recvrecs, nav->cap), 0, PHD_MAX_DEVICES * 8));
	}
	if (e != hipSuccess) {
		(void) hipGetLastError();
		free_sharded(nav);
		return nav->fail(PHD_ERR_DEVICE, std::string("buffers of the sharded step: ") + hipGetErrorString(e));
	}
	nav->sharded_ready = true;
	return PHD_OK;
}

// the local part of a sharded step: the per-particle kernels, then the un-normalised weights stored where the exchange
// reads them (the host's all-gather buffer, or every shard's gathered vector)
static int step_local(phd_navigator* nav, uint8_t onlymapping)
{
	if (nav->P < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_step_local: no particles");
	enter(nav);
	int rc = ensure_sharded(nav);
	if (rc) return rc;
	nav->sharded_used = true;
	nav->timing_now = (nav->timing_step++ % nav->timing_period) == 0;
	StepBufs b = make_bufs(nav);
	rc = launch_map(nav, b, !onlymapping);
	if (rc) return rc;
	// (per-rank host: the export buffer holds P + 1 doubles, the step's status word behind the weights)
	launch_timed(nav, T_PW, nav->stream, false, k_push_weights, dim3((nav->P + 255) / 256), dim3(256), 0, b, (double* const*) nav->d_dst_tab, nav->ndst,
	             nav->push_first, nav->gw_shared ? nav->push_flagslot : nav->P);
	HC(hipGetLastError());
	return PHD_OK;
}

int phd_step_local_async(phd_navigator* nav, uint8_t onlymapping)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_step_local_async");
	HISTORY_UNSUPPORTED(nav, "phd_step_local_async");
	return step_local(nav, onlymapping);
}

void* phd_device_local_weights(phd_navigator* nav)
{
	if (!nav || nav->multi) return nullptr;
	if (ensure_sharded(nav)) return nullptr;
	return nav->d_lw;   // filled by phd_step_local_async, on the handle's stream
}

void* phd_device_global_weights(phd_navigator* nav, int world_particles)
{
	if (!nav || nav->multi || world_particles < 1) return nullptr;
	enter(nav);
	if (ensure_gw(nav, world_particles)) return nullptr;
	return nav->d_gw;
}

// The migration plan from the global source vector: over a grid of workgroups where the vector is long enough to pay for them — its
// counting inside the grid resampling's last launch (`counted`), or as k_plan_count (phd_test_migration_plan: a vector from the
// host), then k_plan_lists —, by one workgroup otherwise (k_plan_migration).
static bool plan_on_grid(const phd_navigator* nav, int Pl, int n)
{
	const long long Pg = (long long) Pl * n;
	return nav->plan_grid_min > 0 && Pg >= nav->plan_grid_min && Pg <= PLAN_GRID_MAXSLOTS && (Pl & 63) == 0 && nav->d_plang != nullptr;
}

// One turn of the grid plan's accumulator sets. The pair's set is chosen before the launches that add to it are enqueued (the
// counting may ride in the grid resampling's last launch); the parity flips when k_plan_lists — the launch that clears the OTHER
// set for the next pair — has been enqueued without error (enqueued()). A turn that ends before that leaves sets nobody will
// clear: both are cleared on the stream, behind whatever was enqueued, and the parity starts over. (use = false: no turn at all —
// the plan of this step does not run over the grid. The clearing's own result is not looked at: a stream that cannot take a memset
// takes no further step either, and the handle's next call reports it.)
struct PlanGridTurn {
	phd_navigator* nav;
	PlanGrid pg;
	bool open;
	PlanGridTurn(phd_navigator* nv, bool use) : nav(nv), open(use)
	{
		std::memset(&pg, 0, sizeof pg);
		if (!use) return;
		const size_t set = plan_grid_set_words(nav);
		int* cur = nav->d_plang + (size_t) nav->plan_par * set;
		int* nxt = nav->d_plang + (size_t) (nav->plan_par ^ 1) * set;
		pg.cnt = cur; pg.used = (unsigned int*) (cur + PHD_MAX_DEVICES * PHD_MAX_DEVICES); pg.bad = cur + set - 1;
		pg.cnt_next = nxt; pg.used_next = (unsigned int*) (nxt + PHD_MAX_DEVICES * PHD_MAX_DEVICES); pg.bad_next = nxt + set - 1;
		pg.wcg = nav->d_plang + 2 * set;
		pg.lcg = pg.wcg + 1024;
	}
	void enqueued() { nav->plan_par ^= 1; open = false; }
	~PlanGridTurn()
	{
		if (!open) return;
		(void) hipMemsetAsync(nav->d_plang, 0, 2 * plan_grid_set_words(nav) * 4, nav->stream);
		nav->plan_par = 0;
	}
	PlanGridTurn(const PlanGridTurn&) = delete;
	PlanGridTurn& operator=(const PlanGridTurn&) = delete;
};

// turn: the caller's, when the plan's counting was part of an earlier launch of it (`counted`); NULL: a turn of this call's own
static int launch_plan(phd_navigator* nav, const StepBufs& b, const int* gsrc, const int* info, const int* lflags, const double* gflags,
                       int Pl, int n, int rank, int* hostcounts, int seq, const double* gw, PlanGridTurn* turn = nullptr, bool counted = false)
{
	if (plan_on_grid(nav, Pl, n)) {
		PlanGridTurn own(nav, turn == nullptr);
		if (!turn) turn = &own;
		const int G = (int) (((long long) Pl * n + 255) / 256);
		if (!counted) hipLaunchKernelGGL(k_plan_count, dim3(G), dim3(256), 0, nav->stream, gsrc, info, lflags, gflags, Pl, n, rank, turn->pg);
		hipLaunchKernelGGL(k_plan_lists, dim3(G), dim3(256), 0, nav->stream, gsrc, info, lflags, gflags, Pl, n, rank, nav->plan, turn->pg, hostcounts, seq, b, gw);
		HC(hipGetLastError());
		turn->enqueued();
		return PHD_OK;
	}
	hipLaunchKernelGGL(k_plan_migration, dim3(1), dim3(1024), plan_lds_bytes(Pl, n), nav->stream, gsrc, info, lflags, gflags, Pl, n, rank, nav->plan,
	                   hostcounts, seq, b, gw);
	HC(hipGetLastError());
	return PHD_OK;
}

// the global part: the resampling kernel on the gathered vector, this rank's weights back into its bank, the plan.
// onlymapping: OnlyMapping keeps the weights and never resamples (PHDNavigator.cs:330-336) — the same kernel with the
// weights taken as they are and resampling off. hostcounts: the plan also writes its counts to pinned host memory.
static int step_global(phd_navigator* nav, int rank, int world_size, double u, uint8_t onlymapping, bool hostcounts, bool from_graw = false)
{
	enter(nav);
	const int Pg = nav->P * world_size;
	nav->last_world_particles = Pg;
	nav->world = world_size; nav->rank = rank;
	int rc = ensure_sharded(nav, hostcounts);
	if (!rc) rc = ensure_gw(nav, Pg);
	if (rc) return rc;
	nav->plan_on_device = !hostcounts;
	StepBufs b = make_bufs(nav);
	// (from_graw: the all-gather landed as [rank][P + 1] (weights | status word): the weights go into the contiguous vector the global
	// kernel takes, the status words behind it — a flag raised on ANY rank then drops the step on every rank alike; done by the
	// resampling's own first launch, or by k_ungather in front of the one-workgroup kernel)
	if (from_graw) nav->d_gflags = nav->d_gw + Pg;
	else if (!nav->gw_shared) nav->d_gflags = nullptr;   // (the host-plan path gathers the weights only: every rank answers for its own flags)
	// (the plan over the grid: its accumulators are chosen here, its counting rides in the grid resampling's last launch when that runs)
	const bool pgrid = plan_on_grid(nav, nav->P, world_size);
	PlanGridTurn turn(nav, pgrid);   // (a return before k_plan_lists is enqueued ends it)
	bool counted = false;
	{
		Timed t(nav, T_NR, nav->stream);
		rc = launch_normalise(nav, b, nav->d_gw, Pg, u, onlymapping ? -1 : 0, onlymapping ? 1 : 0, nav->d_plan, nav->d_info, nullptr, nullptr,
		                      from_graw ? (const double*) nav->d_graw : nullptr, nav->P, world_size, pgrid ? &turn.pg : nullptr, rank, nav->d_gflags, &counted);
	}
	if (rc) return rc;
	int* hc = nullptr;
	if (hostcounts) {
		HC(hipHostGetDevicePointer((void**) &hc, nav->h_counts, 0));
		nav->plan_seq++;
		nav->plan_waiting = true;
	}
	Timed t(nav, T_PL, nav->stream);
	return launch_plan(nav, b, (const int*) nav->d_plan, (const int*) nav->d_info, (const int*) nav->d_flags, nav->d_gflags, nav->P, world_size, rank, hc,
	                   nav->plan_seq, (const double*) nav->d_gw, pgrid ? &turn : nullptr, counted);
}

int phd_step_global_async(phd_navigator* nav, int rank, int world_size, double u_resample)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_step_global_async");
	HISTORY_UNSUPPORTED(nav, "phd_step_global_async");
	if (world_size < 1 || world_size > PHD_MAX_DEVICES || rank < 0 || rank >= world_size) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_step_global: bad rank/world (at most 64 ranks)");
	return step_global(nav, rank, world_size, u_resample, 0, true);
}

// ---- the same step with NOTHING for the host to wait for (round 4): the migrating particles are pushed by the senders,
// straight into their places in the receivers' buffers, from the plan the device made. The host of rank r
//   once:      exchanges the ranks' phd_migration_ipc_export handles and opens them (phd_migration_ipc_open), or — shards in
//              one process — hands in the raw pointers (phd_migration_set_peers)
//   per step:  phd_step_local_async            local kernels; weights | status word into phd_device_local_weights [P + 1]
//              <all-gather of those P + 1 doubles into phd_device_gather_buffer, RCCL>
//              phd_step_global_device_async    un-gather, global resampling, plan — all on the device
//              phd_migration_push_async        k_pack_particles with the peers' buffers as destinations
//              <a one-word all-reduce on the stream: every rank's records have landed>
//              phd_migration_unpack_async      k_finish_sharded
// and never learns whether the step resampled, how many particles moved, or whether a flag dropped it, before phd_sync.
void* phd_device_gather_buffer(phd_navigator* nav, int world_size)
{
	if (!nav || nav->multi || world_size < 1 || world_size > PHD_MAX_DEVICES) return nullptr;
	enter(nav);
	const int need = world_size * (nav->Pcap + 1);
	if (need > nav->grawcap) {
		if (hipStreamSynchronize(nav->stream) != hipSuccess) return nullptr;
		nav->d_graw.reset();
		nav->grawcap = 0;
		if (nav->d_graw.alloc(need) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
		hipMemset(nav->d_graw, 0, (size_t) need * 8);
		nav->grawcap = need;
	}
	return nav->d_graw;
}

int phd_step_global_device_async(phd_navigator* nav, int rank, int world_size, double u_resample, uint8_t onlymapping)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_step_global_device_async");
	HISTORY_UNSUPPORTED(nav, "phd_step_global_device_async");
	if (world_size < 1 || world_size > PHD_MAX_DEVICES || rank < 0 || rank >= world_size) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_step_global_device: bad rank/world (at most 64 ranks)");
	if (!nav->d_graw || nav->grawcap < world_size * (nav->P + 1)) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_step_global_device: no gather buffer (phd_device_gather_buffer(world_size) first)");
	if (!nav->peers_set && world_size > 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_step_global_device: the peers' receive buffers are not known (phd_migration_ipc_open / phd_migration_set_peers first)");
	nav->landing_seq++;
	return step_global(nav, rank, world_size, u_resample, onlymapping, false, true);
}

// How the receiver of a device-path step learns that the migrating particles have landed (phd_migration_push_async ->
// phd_migration_unpack_async):
//   0 (default)  the caller orders the two calls itself — a collective on the stream between them (the one-word all-reduce of
//                rounds 3 - 4), or one stream for all the handles of a process;
//   1            flags: the push ends with a store of the step's number into every peer's receive buffer, the unpack waits (on
//                the device, bounded) for the flags of the ranks it takes records from. No second collective per step. Needs
//                fine-grained receive buffers (phd_migration_recv_is_finegrained): with ordinary device memory a peer's store is
//                only visible at a kernel boundary, and the call is refused.
int phd_migration_set_landing(phd_navigator* nav, int flags)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_migration_set_landing");
	int rc = ensure_sharded(nav, false);
	if (rc) return rc;
	if (flags && !nav->recv_finegrained) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_migration_set_landing: the receive buffer is not fine-grained memory: order push and unpack with a collective instead");
	enter(nav);
	HC(hipStreamSynchronize(nav->stream));
	nav->landing_flags = flags ? 1 : 0;
	if (const char* e = getenv("PHD_LANDING_TIMEOUT_MS")) nav->landing_ticks = std::max(1LL, atoll(e)) * 100000LL;
	return PHD_OK;
}

// the 64-byte hipIpcMemHandle_t of this rank's receive buffer, for the other ranks' processes to open
int phd_migration_ipc_export(phd_navigator* nav, void* handle64, int64_t* buffer_bytes)
{
	if (!nav || !handle64) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_migration_ipc_export");
	int rc = ensure_sharded(nav, false);
	if (rc) return rc;
	static_assert(sizeof(hipIpcMemHandle_t) == 64, "the ABI hands out 64 bytes");
	hipIpcMemHandle_t h;
	HC(hipIpcGetMemHandle(&h, nav->d_recv));
	std::memcpy(handle64, &h, 64);
	if (buffer_bytes) *buffer_bytes = (int64_t) (mig_recv_doubles(nav->recvrecs, nav->cap) * 8);
	return PHD_OK;
}

// recv_buffers[world_size]: where every rank's receive buffer is, as THIS device addresses it (entry `rank` may be NULL:
// the handle's own). Shards in one process pass each other's phd_migration_recv_buffer (with peer access enabled).
int phd_migration_set_peers(phd_navigator* nav, void* const* recv_buffers, int rank, int world_size)
{
	if (!nav || !recv_buffers) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_migration_set_peers");
	if (world_size < 1 || world_size > PHD_MAX_DEVICES || rank < 0 || rank >= world_size) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_migration_set_peers: bad rank/world (at most 64 ranks)");
	int rc = ensure_sharded(nav, false);
	if (rc) return rc;
	std::vector<double*> tab(world_size);
	for (int t = 0; t < world_size; t++) {
		tab[t] = (t == rank) ? nav->d_recv : (double*) recv_buffers[t];
		if (!tab[t]) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_migration_set_peers: the receive buffer of rank " + std::to_string(t) + " is NULL");
	}
	enter(nav);
	HC(hipStreamSynchronize(nav->stream));
	HC(hipMemcpy(nav->d_recv_tab, tab.data(), world_size * sizeof(double*), hipMemcpyHostToDevice));
	nav->peers_set = true;
	nav->world = world_size; nav->rank = rank;
	return PHD_OK;
}

// handles[world_size][64]: every rank's phd_migration_ipc_export, in rank order (the entry of `rank` itself is not opened)
int phd_migration_ipc_open(phd_navigator* nav, const void* handles, int rank, int world_size)
{
	if (!nav || !handles) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_migration_ipc_open");
	if (world_size < 1 || world_size > PHD_MAX_DEVICES || rank < 0 || rank >= world_size) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_migration_ipc_open: bad rank/world (at most 64 ranks)");
	enter(nav);
	// Work in flight on the stream may still store into the mappings of an earlier call: it ends first. From here until
	// phd_migration_set_peers has filled the table again the handle has NO peers — a failure below leaves it that way
	// (phd_step_global_device_async / phd_migration_push_async then refuse), never with a table of closed mappings.
	HC(hipStreamSynchronize(nav->stream));
	nav->peers_set = false;
	for (void* q : nav->ipc_opened) hipIpcCloseMemHandle(q);
	nav->ipc_opened.clear();
	std::vector<void*> ptrs(world_size, nullptr);
	std::vector<void*> opened;
	for (int t = 0; t < world_size; t++) {
		if (t == rank) continue;
		hipIpcMemHandle_t h;
		std::memcpy(&h, (const char*) handles + (size_t) t * 64, 64);
		void* q = nullptr;
		const hipError_t e = hipIpcOpenMemHandle(&q, h, hipIpcMemLazyEnablePeerAccess);
		if (e != hipSuccess) {
			(void) hipGetLastError();
			for (void* o : opened) hipIpcCloseMemHandle(o);   // what this attempt opened
			return nav->fail(PHD_ERR_DEVICE, "phd_migration_ipc_open: the receive buffer of rank " + std::to_string(t) + " cannot be opened: " + hipGetErrorString(e) +
			                 " (the ranks' GPUs must reach each other peer to peer; HSA_ENABLE_IPC_MODE_LEGACY=0 on this pool)");
		}
		opened.push_back(q);
		ptrs[t] = q;
	}
	const int rc = phd_migration_set_peers(nav, ptrs.data(), rank, world_size);
	if (rc) {
		for (void* o : opened) hipIpcCloseMemHandle(o);
		return rc;
	}
	nav->ipc_opened = opened;
	return PHD_OK;
}

// 1: the receive buffer is fine-grained device memory (coherent for the peers storing into it); 0: an ordinary allocation
int phd_migration_recv_is_finegrained(phd_navigator* nav)
{
	if (!nav || nav->multi) return -1;
	if (ensure_sharded(nav, false)) return -1;
	return nav->recv_finegrained ? 1 : 0;
}

// pack, with every record stored straight into its place in its destination's receive buffer (the count and the places are
// the device plan's: a fixed grid strides over the records; nothing runs when the step did not resample or was dropped)
int phd_migration_push_async(phd_navigator* nav)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_migration_push_async");
	if (!nav->sharded_ready || !nav->peers_set) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_migration_push_async: no peers (phd_migration_ipc_open / phd_migration_set_peers, then phd_step_global_device_async)");
	enter(nav);
	if (nav->world <= 1) return PHD_OK;   // (one rank: nothing ever leaves it)
	StepBufs b = make_bufs(nav);
	{
		Timed t(nav, T_PK, nav->stream);
		hipLaunchKernelGGL(k_pack_particles, dim3(std::min(nav->plan.sendcap, 256)), dim3(256), 0, nav->stream, b, nav->plan, nav->world, (double*) nullptr,
		                   (double* const*) nav->d_recv_tab);
		if (nav->landing_flags && nav->world > 1) {
			hipLaunchKernelGGL(k_post_landing, dim3(1), dim3(64), 0, nav->stream, (double* const*) nav->d_recv_tab, nav->world, nav->rank,
			                   mig_landing_offset(nav->recvrecs, nav->cap), nav->landing_seq);
		}
	}
	HC(hipGetLastError());
	return PHD_OK;
}

// Pure host logic (no handle, no device): from the global source vector of a resampling step, which of
// this rank's particles go where and where each of its slots comes from. Both sides derive their lists
// from the same vector, so the sender's order per destination equals the receiver's order per source.
//   send_list : local indices to pack, grouped by destination rank (ascending), then by destination slot
//   dst_code  : per local slot: >= 0 local source index, < 0 -(k + 1) = record k of the receive buffer
// Returns the number of records received.
int phd_plan_migration(const int32_t* gsrc, int Pl, int world_size, int rank, int32_t* send_counts, int32_t* recv_counts,
                       int32_t* send_list, int32_t* dst_code)
{
	// A source particle travels to a rank ONCE, however many of that rank's slots take it: systematic resampling hands a
	// heavy particle to a run of consecutive slots, and the copies of a particle share its map anyway (slot indirection).
	// Sender and receiver both skip a slot whose source equals that of the slot before it (among the slots the two ranks
	// have in common), so their lists agree; a depleted particle set, which is when resampling happens, migrates a small
	// fraction of the records a copy per slot would.
	const int first = rank * Pl;
	for (int r = 0; r < world_size; r++) send_counts[r] = recv_counts[r] = 0;
	int ns = 0;
	for (int r = 0; r < world_size; r++) {
		if (r == rank) continue;
		int prev = -1;
		for (int g = r * Pl; g < (r + 1) * Pl; g++) {
			int s = gsrc[g];
			if (s >= first && s < first + Pl) {
				if (s != prev) {
					send_list[ns++] = s - first;
					send_counts[r]++;
				}
				prev = s;
			}
		}
	}
	for (int i = 0; i < Pl; i++) {
		int s = gsrc[first + i];
		if (s >= first && s < first + Pl) dst_code[i] = s - first;
	}
	int slot = 0;
	for (int r = 0; r < world_size; r++) {
		if (r == rank) continue;
		int prev = -1;
		for (int i = 0; i < Pl; i++) {
			int s = gsrc[first + i];
			if (s >= r * Pl && s < (r + 1) * Pl) {
				if (s != prev) {
					slot++;
					recv_counts[r]++;
				}
				dst_code[i] = -slot;   // record slot - 1 of the receive buffer
				prev = s;
			}
		}
	}
	return slot;
}

// Test surface of the device plan: k_plan_migration on a caller-supplied global source vector (the host statement above is
// its reference in the tests). Arrays as phd_plan_migration's, plus fslot[<= Pl] (the OUT-bank slots of the arriving
// records) and send_dst[<= Pl + 64][2] (destination rank, record number in its receive buffer). *status <- MIG_*;
// returns PHD_OK when the kernel ran.
int phd_test_migration_plan(phd_navigator* nav, const int32_t* gsrc, int particles_per_rank, int world_size, int rank, int resampled,
                            int32_t* send_counts, int32_t* recv_counts, int32_t* send_list, int32_t* dst_code, int32_t* fslot,
                            int32_t* send_dst, int32_t* nsend, int32_t* nrecv, int32_t* status)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	if (nav->multi) nav = multi_shard0(nav);
	const int Pl = particles_per_rank, n = world_size;
	if (!gsrc || Pl < 1 || Pl > nav->Pcap || n < 1 || n > PHD_MAX_DEVICES || rank < 0 || rank >= n || !send_counts || !recv_counts || !send_list || !dst_code ||
	    !fslot || !send_dst || !nsend || !nrecv || !status) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_test_migration_plan: sizes out of range (particles_per_rank <= max_particles, world_size <= 64)");
	}
	enter(nav);
	int rc = ensure_sharded(nav);
	if (rc) return rc;
	HC(hipStreamSynchronize(nav->stream));
	DevBuf<int> d_g;
	HC(d_g.alloc((size_t) Pl * n + 4));
	int* d_i = d_g + (size_t) Pl * n;   // info[2], a clear status word
	const int info[3] = {0, resampled ? 1 : 0, 0};
	hipError_t e = hipMemcpy(d_g, gsrc, (size_t) Pl * n * 4, hipMemcpyHostToDevice);
	if (e == hipSuccess) e = hipMemcpy(d_i, info, 12, hipMemcpyHostToDevice);
	if (e == hipSuccess) {
		rc = launch_plan(nav, make_bufs(nav), (const int*) d_g, (const int*) d_i, (const int*) (d_i + 2), (const double*) nullptr, Pl, n, rank, (int*) nullptr, 0,
		                 (const double*) nullptr);
		if (rc) return rc;
		e = hipStreamSynchronize(nav->stream);
	}
	std::vector<int> c(mig_word(n, MC_DEVICE_WORDS));
	if (e == hipSuccess) e = hipMemcpy(c.data(), nav->plan.counts, c.size() * 4, hipMemcpyDeviceToHost);
	if (e != hipSuccess) return nav->fail(PHD_ERR_DEVICE, std::string("phd_test_migration_plan: ") + hipGetErrorString(e));
	for (int r = 0; r < n; r++) { send_counts[r] = c[r]; recv_counts[r] = c[n + r]; }
	*nsend = c[mig_word(n, MC_NSEND)]; *nrecv = c[mig_word(n, MC_NRECV)]; *status = c[mig_word(n, MC_STATUS)];
	if (*status == MIG_OK && resampled) {
		std::vector<long long> sd((size_t) std::max(*nsend, 1));
		HC(hipMemcpy(dst_code, nav->plan.code, (size_t) Pl * 4, hipMemcpyDeviceToHost));
		if (*nrecv > 0) HC(hipMemcpy(fslot, nav->plan.fslot, (size_t) *nrecv * 4, hipMemcpyDeviceToHost));
		if (*nsend > 0) {
			HC(hipMemcpy(send_list, nav->plan.sendlist, (size_t) *nsend * 4, hipMemcpyDeviceToHost));
			HC(hipMemcpy(sd.data(), nav->plan.senddst, (size_t) *nsend * 8, hipMemcpyDeviceToHost));
			for (int k = 0; k < *nsend; k++) { send_dst[2 * k] = (int32_t) (sd[k] >> 32); send_dst[2 * k + 1] = (int32_t) (sd[k] & 0xffffffffll); }
		}
	}
	return PHD_OK;
}

// The split sizes of the exchange. The plan itself was made on the device behind the resampling kernel
// (k_plan_migration); its counts arrive in pinned host memory, and the host waits for the word written behind them — no
// stream synchronisation, no copy command, and nothing of the size of the particle set crosses.
int phd_migration_plan(phd_navigator* nav, int rank, int world_size, int32_t* send_counts, int32_t* recv_counts)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_migration_plan");
	if (world_size < 1 || rank < 0 || rank >= world_size || !send_counts || !recv_counts) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_migration_plan: bad arguments");
	if (!nav->plan_waiting || world_size != nav->world || rank != nav->rank) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_migration_plan: call phd_step_global_async(rank, world_size) first");
	enter(nav);
	const int n = world_size;
	volatile int* hc = nav->h_counts;
	const auto t0 = std::chrono::steady_clock::now();
	for (long spins = 0; hc[mig_word(n, MC_SEQ)] != nav->plan_seq; spins++) {
		__builtin_ia32_pause();
		if ((spins & 0xfff) == 0xfff && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) {
			// (a device that never gets there: report what the stream says rather than spin for ever)
			HC(hipStreamSynchronize(nav->stream));
			if (hc[mig_word(n, MC_SEQ)] != nav->plan_seq) return nav->fail(PHD_ERR_DEVICE, "phd_migration_plan: the plan kernel did not report");
		}
	}
	__atomic_thread_fence(__ATOMIC_ACQUIRE);
	nav->plan_waiting = false;
	const int status = hc[mig_word(n, MC_STATUS)];
	for (int r = 0; r < n; r++) { send_counts[r] = hc[r]; recv_counts[r] = hc[n + r]; }
	nav->nsend = hc[mig_word(n, MC_NSEND)]; nav->nrecv = hc[mig_word(n, MC_NRECV)];
	if (status == MIG_DROPPED) {
		// a kernel of the local step raised a flag: the step is dropped before anything rotates (the caller must not go on to
		// pack / unpack — if it does, those kernels find the same status and leave the state alone; the state is the one
		// before phd_step_local_async)
		nav->h_flags = hc[mig_word(n, MC_FLAGS)];
		hipMemsetAsync(nav->d_flags, 0, 4, nav->stream);
		return check_flags(nav);
	}
	if (status == MIG_BAD) return nav->fail(PHD_ERR_GENERIC, "phd_migration_plan: the gathered source vector is not a resampling result (were the weights of all ranks gathered?)");
	if (status == MIG_OVERFLOW) return nav->fail(PHD_ERR_CAPACITY, "phd_migration_plan: more migrating particles than the send list holds");
	nav->h_info[0] = hc[mig_word(n, MC_BEST)]; nav->h_info[1] = hc[mig_word(n, MC_RESAMPLED)];
	return PHD_OK;
}

// Did the last global step resample? As the host knows it from phd_migration_plan (per-rank host) — identical on every
// rank, so all of them may skip the exchange together when it did not. -1: not known (no plan waited for yet).
int phd_last_resampled(phd_navigator* nav)
{
	if (!nav || nav->multi || !nav->sharded_used || nav->plan_waiting) return -1;
	return nav->h_info[1] ? 1 : 0;
}

void* phd_migration_send_buffer(phd_navigator* nav, int64_t* bytes_per_particle)
{
	if (!nav || nav->multi || ensure_sharded(nav)) return nullptr;
	if (bytes_per_particle) *bytes_per_particle = (int64_t) mig_rec_doubles(nav->cap) * 8;
	return nav->d_send;   // (a fixed address for the life of the handle)
}

void* phd_migration_recv_buffer(phd_navigator* nav) { return (nav && !nav->multi && !ensure_sharded(nav)) ? nav->d_recv : nullptr; }

// grid of k_pack_particles / its like: the records are counted on the device, a fixed grid strides over them
static int pack_grid(const phd_navigator* nav) { return std::min(nav->plan.sendcap, 1024); }

int phd_migration_pack_async(phd_navigator* nav)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_migration_pack_async");
	enter(nav);
	if (!nav->sharded_ready || nav->plan_on_device) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_migration_pack_async: no plan known to the host (phd_step_global_async, phd_migration_plan first)");
	if (nav->nsend == 0) return PHD_OK;   // (the per-rank host knows the counts)
	StepBufs b = make_bufs(nav);
	launch_timed(nav, T_PK, nav->stream, false, k_pack_particles, dim3(std::min(nav->nsend, pack_grid(nav))), dim3(256), 0, b, nav->plan, nav->world,
	             (double*) nav->d_send, (double* const*) nullptr);
	HC(hipGetLastError());
	return PHD_OK;
}

// the end of a sharded step: arrivals unpacked, small arrays gathered, roles rotated — all read from the device plan
static int step_finish(phd_navigator* nav)
{
	enter(nav);
	StepBufs b = make_bufs(nav);
	int* sel_next = nav->d_sel + (nav->parity ^ 1) * SEL_STRIDE;
	nav->d_res_slots = nav->d_mslot;
	{
		Timed t(nav, T_GR, nav->stream);
		if (nav->landing_flags && nav->plan_on_device && nav->world > 1) {   // one wave waits, in front of the launch that reads
			const unsigned long long* landing = (const unsigned long long*) (nav->d_recv + mig_landing_offset(nav->recvrecs, nav->cap));
			hipLaunchKernelGGL(k_wait_landing, dim3(1), dim3(64), 0, nav->stream, nav->plan, nav->world, landing, nav->landing_seq, nav->landing_ticks, nav->d_flags);
		}
		hipLaunchKernelGGL(k_finish_sharded, dim3(nav->P), dim3(256), 0, nav->stream, b, nav->plan, nav->world, (const double*) nav->d_recv,
		                   1.0 / (double) nav->last_world_particles, sel_next, nav->frozen ? 1 : 0, nav->d_inslot, nav->d_mslot);
	}
	HC(hipGetLastError());
	nav->parity ^= 1;
	nav->stage_valid = false;
	nav->sel_host_valid = false;   // the rotation depends on the plan's status and the resampling flag, known on the device
	return PHD_OK;
}

int phd_migration_unpack_async(phd_navigator* nav)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_migration_unpack_async");
	if (!nav->sharded_ready) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_migration_unpack_async: no plan (phd_step_global_async first)");
	return step_finish(nav);
}

// Lend the handle a stream of the host (e.g. the framework's current stream) so that the library's kernels and
// the host's collectives are ordered by the stream itself (NULL = the default stream); lend = 0 returns to the handle's own.
int phd_set_stream(phd_navigator* nav, void* stream, uint8_t lend)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_set_stream");
	enter(nav);
	HC(hipStreamSynchronize(nav->stream));
	nav->stream = lend ? (hipStream_t) stream : nav->own_stream;   // a NULL lent stream is the legacy default stream
	return PHD_OK;
}

// (Last in the file: the two kernels are instantiated here, behind every other kernel of the code object, and move none of them.)
// A mapping-only step that particle slot `held` sits out (phd_hold.h): its mixture is copied out of the current state in front of
// the step and back into the current state behind it. Nothing of the step itself knows. Both copies run on `stream`; with two
// sub-range streams the held step takes the fork / join order on both sides (pipe_ok = false: the stream the step forks from is
// behind everything of the step before — its end left both streams ordered behind k_normalise_resample —, and the step's end
// leaves `stream` behind everything of this one), and so does the step behind it. held == -1 is phd_step_async as it stands.
int phd_step_hold_async(phd_navigator* nav, int held)
{
	if (!nav) return PHD_ERR_BAD_ARGUMENT;
	MULTI_UNSUPPORTED(nav, "phd_step_hold_async");
	if (nav->P < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_step_hold_async: no particles (call phd_reset first)");
	if (held < -1 || held >= nav->P) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_step_hold_async: `held` is a particle slot of the current state, or -1");
	if (nav->frozen) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_step_hold_async: frozen mode (the state does not advance: nothing to hold)");
	if (nav->sharded_used) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_step_hold_async: not available on a handle that has run sharded steps");
	if (held < 0) return phd_step_async(nav, 1, 0.0);
	if (!nav->d_hold) {
		hipSetDevice(nav->device);
		DevBuf<double> rec; DevBuf<int> cnt;
		hipError_t e = rec.alloc((size_t) nav->cap * MIX_REC);
		if (e == hipSuccess) e = cnt.alloc(1);
		if (e != hipSuccess) return nav->fail(PHD_ERR_DEVICE, std::string("phd_step_hold_async: allocation: ") + hipGetErrorString(e));
		nav->d_hold = std::move(rec); nav->d_hold_count = std::move(cnt);
	}
	enter(nav);
	{
		StepBufs b = make_bufs(nav);   // the roles in front of the step
		hipLaunchKernelGGL((k_hold_save<int>), dim3(1), dim3(256), 0, nav->stream, b, held, nav->Pcap, (double*) nav->d_hold, (int*) nav->d_hold_count);
		HC(hipGetLastError());
	}
	int rc = phd_step_async(nav, 1, 0.0);
	if (rc) return rc;
	{
		StepBufs b = make_bufs(nav);   // ... and behind it (the parity has advanced)
		hipLaunchKernelGGL((k_hold_restore<int>), dim3(1), dim3(256), 0, nav->stream, b, held, nav->Pcap, (const double*) nav->d_hold, (const int*) nav->d_hold_count);
		HC(hipGetLastError());
	}
	nav->pipe_ok = false;   // the restore is on `stream` alone: the next step forks behind it
	return PHD_OK;
}

}  // extern "C"

#include "phd_multi.inc"
