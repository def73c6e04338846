// phd_guesses.h — the starting guesses of the pose searches of many frames (phd_quasi_guesses_multi): the guess loop of
// LoopyPHDNavigator.GuidedFitMixture (LoopyPHDNavigator.cs:789-797) for every frame of UpdateMessagesFromMap side by side. For
// every (landmark of the map estimate, measurement) pair of a PROBLEM (phd_ascent_multi.h) the pose that explains the pair
// (PRM3DMeasurer.FitToMeasurement, PRM3DMeasurer.cs:221-243), kept when it lies within `radius` of the problem's initial pose
// (Pose3D.Subtract, the `< 0.5 * 0.5` of :793). monorfs_amd/loopy.py states the formulas: fit_to_measurement, vector_rotator,
// pose3d_subtract with _qlog; everything here is FP64 without contraction.
//
// One lane per pair, tiles of 256 pairs of ONE problem, the grid over (problem, tile) — a call of few frames still fills more
// than a handful of CUs, a workgroup beyond its problem's last tile leaves at once —; pair i of a problem is landmark i / M,
// measurement i % M: landmark-major, the reference's order. The chain of a call:
//   k_guess_count    the fit and the test per lane; one count per tile (ballot and popcount per wave, the 4 waves summed in order)
//   k_guess_offsets  one workgroup: the exclusive scan of the tile counts and guess_offsets (every problem's list starts with its
//                    pose0, so problem q's list begins q places behind the pairs before it)
//   (the host reads guess_offsets: the total decides the capacity rule and the size of the output buffer)
//   k_guess_emit     the fit and the test again, by the same function — no per-pair flag goes through memory —, every passing
//                    pair written at tile offset + rank within the tile: pairs2, guesses6, poses7 = Add(lin, guess), its problem;
//                    tile 0 of a problem also writes its pose0 guess and the far pose it is evaluated at
//   (k_multi_setll over the far poses and the guesses, in chunks)
// What is the same for the 256 lanes of a workgroup — the linearisation pose, the initial pose, its conjugate rotation matrix —
// is made by one lane and staged in LDS. No loop bound depends on data, no kernel waits for another workgroup, every index is
// checked against its count before it is used.
#pragma once
#include "phd_ascent_multi.h"

#define PHD_GUESS_TILE 256

struct GuessBufs {
	int np;                       // problems
	int ntiles;                   // tiles of all problems
	int capacity;                 // guesses the per-guess arrays hold (k_guess_emit)
	double focal, radius2;
	const int* lm_off;            // [np + 1]
	const int* z_off;             // [np + 1]
	const int* tile_first;        // [np + 1] first tile of problem q; problem q has tile_first[q + 1] - tile_first[q] = ceil(J M / 256)
	const double* lm;             // [sum J][3]
	const double* z;              // [sum M][3]
	const double* lin;            // [np][7]
	const double* pose0;          // [np][6]
	const double* far7;           // [7]
	int* tile_count;              // [ntiles]
	int* tile_scan;               // [ntiles + 1] exclusive scan of tile_count, the sum behind it
	int* goff;                    // [np + 1] guess_offsets
	// per evaluated pose: the far pose of every problem first, then the guesses (k_guess_emit)
	int*    problem_of;           // [np + capacity]
	double* poses7;               // [np + capacity][7]
	int*    pairs2;               // [capacity][2]
	double* guesses6;             // [capacity][6]
};

struct GuessFrame {               // what a workgroup stages once (LDS)
	double lin[7];                // the linearisation pose
	double init[7];               // initpose = Add(lin, pose0)
	double rc[9];                 // ToMatrix(conj(initpose rotation)), Quaternion.cs:327-342
	double pose0[6];
};

__device__ __forceinline__ Quat4 quat_conj(const Quat4& q) { return Quat4{q.w, -q.x, -q.y, -q.z}; }

// Pose3D.Subtract (Pose3D.cs:296-308) as loopy.py::pose3d_subtract states it: conj(qo) dx qo, 2 Log(conj(qo) q)
__device__ __forceinline__ void guess_pose_subtract(const double x[3], const Quat4& q, const double* __restrict__ origin, double d[6])
{
	PHD_REF_ARITH
	const Quat4 qo{origin[3], origin[4], origin[5], origin[6]};
	const Quat4 qc = quat_conj(qo);
	const Quat4 dq = quat_mul(qc, q);
	const Quat4 dx = quat_mul(quat_mul(qc, Quat4{0.0, x[0] - origin[0], x[1] - origin[1], x[2] - origin[2]}), qo);
	d[0] = dx.x; d[1] = dx.y; d[2] = dx.z;
	// Quaternion.Log, Quaternion.cs:204-218: normalised, acos of the clamped w, zero below 1e-12
	const double n = sqrt(dq.w * dq.w + dq.x * dq.x + dq.y * dq.y + dq.z * dq.z);
	const double w = dq.w / n, vx = dq.x / n, vy = dq.y / n, vz = dq.z / n;
	const double phi = acos(fmin(1.0, fmax(-1.0, w)));
	const double mag = sqrt(vx * vx + vy * vy + vz * vz);
	if (mag < 1e-12) { d[3] = 0.0; d[4] = 0.0; d[5] = 0.0; }
	else { d[3] = 2.0 * (phi * (vx / mag)); d[4] = 2.0 * (phi * (vy / mag)); d[5] = 2.0 * (phi * (vz / mag)); }
}

// The fit of one pair and its test: FitToMeasurement at the initial pose, Subtract against it, |d|^2 < radius^2 (false on NaN:
// a landmark at the pose's location or opposite the measurement direction makes no guess). guess6: Subtract against the
// linearisation pose, written only when the pair passes. BOTH passes call this, so they agree on every pair.
__device__ __forceinline__ bool guess_fit(const GuessFrame& f, double focal, double radius2, const double* __restrict__ lm3, const double* __restrict__ z3, double guess6[6])
{
	PHD_REF_ARITH
	const double lx = lm3[0], ly = lm3[1], lz = lm3[2];
	const double dx = lx - f.init[0], dy = ly - f.init[1], dz = lz - f.init[2];
	const double ax = f.rc[0] * dx + f.rc[1] * dy + f.rc[2] * dz;
	const double ay = f.rc[3] * dx + f.rc[4] * dy + f.rc[5] * dz;
	const double az = f.rc[6] * dx + f.rc[7] * dy + f.rc[8] * dz;
	const double px = z3[0], py = z3[1], range = z3[2];
	const double m2 = range / sqrt(1.0 + (px * px + py * py) / (focal * focal));
	const double m0 = px * m2 / focal, m1 = py * m2 / focal;
	const double an = sqrt(ax * ax + ay * ay + az * az), mn = sqrt(m0 * m0 + m1 * m1 + m2 * m2);
	const double a0 = ax / an, a1 = ay / an, a2 = az / an, b0 = m0 / mn, b1 = m1 / mn, b2 = m2 / mn;
	// Quaternion.VectorRotator, Quaternion.cs:281-284
	Quat4 al{1.0 + (a0 * b0 + a1 * b1 + a2 * b2), a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0};
	const double aln = sqrt(al.w * al.w + al.x * al.x + al.y * al.y + al.z * al.z);
	al = Quat4{al.w / aln, al.x / aln, al.y / aln, al.z / aln};
	const Quat4 r = quat_mul(quat_conj(al), Quat4{f.init[3], f.init[4], f.init[5], f.init[6]});
	const double w = r.w, x = r.x, y = r.y, z = r.z;   // ToMatrix of the rotation as multiplied, the normalisation is new Pose3D's
	double loc[3];
	loc[0] = lx - ((1.0 - 2.0 * (y * y + z * z)) * m0 + (2.0 * (x * y - z * w)) * m1 + (2.0 * (x * z + y * w)) * m2);
	loc[1] = ly - ((2.0 * (x * y + z * w)) * m0 + (1.0 - 2.0 * (x * x + z * z)) * m1 + (2.0 * (y * z - x * w)) * m2);
	loc[2] = lz - ((2.0 * (x * z - y * w)) * m0 + (2.0 * (y * z + x * w)) * m1 + (1.0 - 2.0 * (x * x + y * y)) * m2);
	const double rn = sqrt(w * w + x * x + y * y + z * z);
	const Quat4 q{w / rn, x / rn, y / rn, z / rn};
	double d[6];
	guess_pose_subtract(loc, q, f.init, d);
	const double dist2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3] + d[4] * d[4] + d[5] * d[5];
	if (!(dist2 < radius2)) return false;
	guess_pose_subtract(loc, q, f.lin, guess6);
	return true;
}

// one lane makes what the workgroup shares; the caller's barrier publishes it
__device__ __forceinline__ void guess_stage(const GuessBufs& g, int q, GuessFrame* f)
{
	PHD_REF_ARITH
#pragma unroll
	for (int k = 0; k < 7; k++) f->lin[k] = g.lin[(size_t) q * 7 + k];
#pragma unroll
	for (int k = 0; k < 6; k++) f->pose0[k] = g.pose0[(size_t) q * 6 + k];
	ascent_pose_add(f->lin, f->pose0, f->init);
	const double w = f->init[3], x = -f->init[4], y = -f->init[5], z = -f->init[6];
	f->rc[0] = 1.0 - 2.0 * (y * y + z * z); f->rc[1] = 2.0 * (x * y - z * w);       f->rc[2] = 2.0 * (x * z + y * w);
	f->rc[3] = 2.0 * (x * y + z * w);       f->rc[4] = 1.0 - 2.0 * (x * x + z * z); f->rc[5] = 2.0 * (y * z - x * w);
	f->rc[6] = 2.0 * (x * z - y * w);       f->rc[7] = 2.0 * (y * z + x * w);       f->rc[8] = 1.0 - 2.0 * (x * x + y * y);
}

// The pair of this lane in tile `t` of problem q, fitted: whether it passes, its (landmark, measurement) and guess. Every index
// is below its count: q < np by the grid, j < J and m < M by i < J M.
__device__ __forceinline__ bool guess_lane(const GuessBufs& g, const GuessFrame& f, int q, int t, int tid, int& j, int& m, double guess6[6])
{
	const int l0 = g.lm_off[q], J = g.lm_off[q + 1] - l0, z0 = g.z_off[q], M = g.z_off[q + 1] - z0;
	const long long i = (long long) t * PHD_GUESS_TILE + tid;
	j = -1; m = -1;
	if (J <= 0 || M <= 0 || i >= (long long) J * M) return false;
	j = (int) (i / M); m = (int) (i - (long long) j * M);
	return guess_fit(f, g.focal, g.radius2, g.lm + 3 * (size_t) (l0 + j), g.z + 3 * (size_t) (z0 + m), guess6);
}

__global__ __launch_bounds__(256) void k_guess_count(const GuessBufs g)
{
	__shared__ GuessFrame f;
	__shared__ int wc[4];
	const int q = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
	if (q >= g.np) return;
	const int t0 = g.tile_first[q], nt = g.tile_first[q + 1] - t0;
	if (t >= nt || t0 + t >= g.ntiles) return;   // (uniform: the whole workgroup leaves)
	if (tid == 0) guess_stage(g, q, &f);
	__syncthreads();
	int j, m;
	double guess6[6];
	const bool pass = guess_lane(g, f, q, t, tid, j, m, guess6);
	const unsigned long long b = ballot64(pass);
	if ((tid & 63) == 0) wc[tid >> 6] = __popcll(b);
	__syncthreads();
	if (tid == 0) g.tile_count[t0 + t] = wc[0] + wc[1] + wc[2] + wc[3];
}

// One workgroup. Lane i owns the tiles [i c, (i + 1) c), c = ceil(ntiles / 256): its sum, the sums of the lanes before it in
// order, its tiles' exclusive offsets. Then guess_offsets per problem.
__global__ __launch_bounds__(256) void k_guess_offsets(const GuessBufs g)
{
	__shared__ int part[256];
	const int tid = threadIdx.x;
	const int c = (g.ntiles + 255) / 256;
	const int first = min(g.ntiles, tid * c), last = min(g.ntiles, first + c);
	int sum = 0;
	for (int i = first; i < last; i++) sum += g.tile_count[i];
	part[tid] = sum;
	__syncthreads();
	int before = 0;
	for (int k = 0; k < 256; k++) before += (k < tid) ? part[k] : 0;
	for (int i = first; i < last; i++) { g.tile_scan[i] = before; before += g.tile_count[i]; }
	if (tid == 255) g.tile_scan[g.ntiles] = before;   // (lane 255's range ends at ntiles, empty or not: `before` is the whole sum)
	__syncthreads();
	for (int q = tid; q <= g.np; q += 256) {
		const int tq = min(max(g.tile_first[q], 0), g.ntiles);
		g.goff[q] = g.tile_scan[tq] + q;
	}
}

__global__ __launch_bounds__(256) void k_guess_emit(const GuessBufs g)
{
	__shared__ GuessFrame f;
	__shared__ int wc[4];
	const int q = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	if (q >= g.np) return;
	const int t0 = g.tile_first[q], nt = g.tile_first[q + 1] - t0;
	if (t > 0 && (t >= nt || t0 + t >= g.ntiles)) return;   // (tile 0 of every problem runs: the pose0 guess is its own)
	if (tid == 0) guess_stage(g, q, &f);
	__syncthreads();
	const int begin = g.goff[q], end = g.goff[q + 1];
	if (t == 0 && tid < 7) g.poses7[(size_t) q * 7 + tid] = g.far7[tid];   // evaluated pose q: the far pose against problem q
	if (t == 0 && tid == 0) g.problem_of[q] = q;
	if (t == 0 && tid == 0 && begin >= 0 && begin < end && begin < g.capacity) {
		g.pairs2[2 * (size_t) begin] = -1; g.pairs2[2 * (size_t) begin + 1] = -1;
#pragma unroll
		for (int k = 0; k < 6; k++) g.guesses6[(size_t) begin * 6 + k] = f.pose0[k];
#pragma unroll
		for (int k = 0; k < 7; k++) g.poses7[(size_t) (g.np + begin) * 7 + k] = f.init[k];   // (Add(lin, pose0) by ascent_pose_add: guess_stage)
		g.problem_of[g.np + begin] = q;
	}
	if (t >= nt || t0 + t >= g.ntiles) return;   // (a problem without pairs)
	int j, m;
	double guess6[6];
	const bool pass = guess_lane(g, f, q, t, tid, j, m, guess6);
	const unsigned long long b = ballot64(pass);
	if (lane == 0) wc[wv] = __popcll(b);
	__syncthreads();
	if (!pass) return;
	int rank = __popcll(b & ((1ull << lane) - 1ull));
#pragma unroll
	for (int k = 0; k < 3; k++) rank += (k < wv) ? wc[k] : 0;
	const long long e = (long long) g.tile_scan[t0 + t] + q + 1 + rank;
	if (e <= begin || e >= end || e >= g.capacity) return;
	g.pairs2[2 * (size_t) e] = j; g.pairs2[2 * (size_t) e + 1] = m;
#pragma unroll
	for (int k = 0; k < 6; k++) g.guesses6[(size_t) e * 6 + k] = guess6[k];
	ascent_pose_add(f.lin, guess6, g.poses7 + (size_t) (g.np + e) * 7);
	g.problem_of[g.np + e] = q;
}
