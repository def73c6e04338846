// phd_poseerror.h — the pose-error series of the reference's post-analysis over the trajectory log (phd_pose_error):
// Plot.LocationError / RotationError / OdoLocationError / OdoRotationError (postanalysis/Plot.cs:293-456) in the three history
// modes of Plot.poseError (:325-369), everything in FP64. monorfs_amd/host/PoseError.hpp is the same metric on the host, written
// sequentially in the reference's order, and states the formulas.
//
// One workgroup of 256 threads per path: in Timed mode one per estimate (the best particle's whole path as of its entry), in
// Smooth and Filter mode one workgroup in all.
//   1. the path's slots, one 16-bit word per entry, into LDS: wave 0 walks the ancestry backwards as k_hist_trace does (a ballot
//      of the dirty words per 64 entries, one dependent load per resampled entry). Filter mode has no path: every entry's slot
//      is its own estimate's.
//   2. all four waves stride over the entries; a thread gathers the poses it needs from the log by the slots in LDS and the
//      truth rows beside them and evaluates the errors. Timed mode adds them up: per-thread partials in the order of the
//      stride, then one fixed tree over the 256 partials in LDS — the same bits whatever the grid and from run to run.
//      Smooth and Filter mode write the per-entry values.
//
// LDS of a workgroup: 8 KB of partials (static) and the slot row, 2 bytes per entry of the log (dynamic, at most 48 KB for
// PHD_POSEERR_MAX entries). 16-bit slots hold any slot of a handle of up to 65 536 particles; the host refuses larger ones.
// Every loop is bounded by a number known at launch (L, 64). Every slot read from device memory is clamped into [0, P) before
// it is used as an index. No atomics, no waiting on another workgroup.
#pragma once
#include "phd_maplog.h"

#define PHD_POSEERR_MAX 24576        // entries of the log (include/phdhip.h: PHD_POSE_ERROR_MAX): a slot row of 48 KB
#define PHD_POSEERR_MAX_PARTICLES 65536
#define PHD_POSEERR_ODO 10           // the odometry series compares entry k with entry k - 10 (Plot.cs:414)

struct PeQ { double w, x, y, z; };
struct PePose { double x, y, z; PeQ q; };

__device__ __forceinline__ PeQ pe_qmul(const PeQ& a, const PeQ& b)   // Quaternion.cs:295-301
{
	return PeQ{a.w * b.w - (a.x * b.x + a.y * b.y + a.z * b.z), a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
	           a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ PeQ pe_qconj(const PeQ& q) { return PeQ{q.w, -q.x, -q.y, -q.z}; }
__device__ __forceinline__ PeQ pe_qnormalize(const PeQ& q)
{
	const double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
	return PeQ{q.w / n, q.x / n, q.y / n, q.z / n};
}
__device__ __forceinline__ double pe_clamp1(double v) { return fmin(1.0, fmax(-1.0, v)); }

// Pose3D.FromState (Pose3D.cs:142-162): the quaternion scaled to norm 1
__device__ __forceinline__ PePose pe_load(const double* __restrict__ p)
{
	const double x = p[0], y = p[1], z = p[2], qw = p[3], qx = p[4], qy = p[5], qz = p[6];
	const double a = 1.0 / sqrt(qw * qw + qx * qx + qy * qy + qz * qz);
	return PePose{x, y, z, PeQ{a * qw, a * qx, a * qy, a * qz}};
}

// FromLinear(pose ⊖ origin): Pose3D.Subtract (Pose3D.cs:297-308), then Identity.Add of it (:282-291), whose rotation of the
// location by the identity changes nothing
__device__ __forceinline__ PePose pe_relative(const PePose& pose, const PePose& origin)
{
	const PeQ qo = origin.q;
	const PeQ dq = pe_qnormalize(pe_qmul(pe_qconj(qo), pose.q));
	const PeQ dx = pe_qmul(pe_qmul(pe_qconj(qo), PeQ{0.0, pose.x - origin.x, pose.y - origin.y, pose.z - origin.z}), qo);
	const double phi = acos(pe_clamp1(dq.w));   // Quaternion.Log, Quaternion.cs:203-217
	const double mag = sqrt(dq.x * dq.x + dq.y * dq.y + dq.z * dq.z);
	double r0 = 0.0, r1 = 0.0, r2 = 0.0;
	if (!(mag < 1e-12)) { r0 = 2 * phi * (dq.x / mag); r1 = 2 * phi * (dq.y / mag); r2 = 2 * phi * (dq.z / mag); }
	const double l0 = 0.5 * r0, l1 = 0.5 * r1, l2 = 0.5 * r2;
	const double half = sqrt(l0 * l0 + l1 * l1 + l2 * l2);
	PeQ q{1.0, 0.0, 0.0, 0.0};
	if (!(half < 1e-12)) {   // Quaternion.Exp, Quaternion.cs:185-196
		const double s = sin(half);
		q = pe_qnormalize(PeQ{cos(half), s * (l0 / half), s * (l1 / half), s * (l2 / half)});
	}
	return PePose{dx.x, dx.y, dx.z, q};
}

// diffloc and diffrot (Plot.cs:445-456) of FromLinear(ga ⊖ gb) against FromLinear(ea ⊖ eb)
__device__ __forceinline__ void pe_errors(const PePose& ga, const PePose& gb, const PePose& ea, const PePose& eb, double* loc, double* rot)
{
	const PePose d = pe_relative(pe_relative(ga, gb), pe_relative(ea, eb));
	*loc = sqrt(d.x * d.x + d.y * d.y + d.z * d.z);
	const double pi = 3.14159265358979323846;
	const double raw = 2 * acos(pe_clamp1(d.q.w));   // Quaternion.Angle, Quaternion.cs:71-74
	double normal = fmod(raw + pi, 2 * pi);          // Util.NormalizeAngle, Util.cs:79-87
	normal = (normal >= 0) ? normal : normal + 2 * pi;
	*rot = fabs(normal - pi);
}

// the slot whose path is the estimate at entry k: the host's list, or the best of the newest map-log entry appended before
// trajectory entry k (sel[k] is then the map log's length at that moment; 0: slot 0)
template <class Entry>
__device__ __forceinline__ int pe_slot_of(const int* __restrict__ sel, int from_marks, const Entry* __restrict__ mlentry, int mlog_len, int k, int P)
{
	int s = sel[k];
	if (from_marks) {
		const int mark = s > mlog_len ? mlog_len : s;
		s = mark >= 1 ? mlentry[mark - 1].best : 0;
	}
	return hist_clamp(s, P);
}

// mode: PHD_POSE_ERROR_TIMED 0 | _SMOOTH 1 | _FILTER 2.
//   Timed: grid L - first, workgroup b is the estimate i = first + b; out[q * cap + b], q = loc | rot | odoloc | odorot, the
//          mean of the series from start[i] on.
//   Smooth: grid 1, the path of the slot at entry L - 1; out[q * cap + j] the series themselves (L values, 1 + max(0, L - 10)
//          of the two odometry series).
//   Filter: grid 1, position j is entry first + j with its own slot; as Smooth over L - first positions.
// The launch's dynamic LDS is the slot row: 2 bytes per entry of the log, L of them.
// A template for its place in the code object alone, as k_maplog_append is (phd_maplog.h).
template <class Entry>
__global__ __launch_bounds__(256) void k_pose_error(const double* __restrict__ pose, const int* __restrict__ parent, const int* __restrict__ dirty, int L, int P, int Ps,
                                                    const double* __restrict__ truth, const int* __restrict__ sel, int from_marks, const Entry* __restrict__ mlentry,
                                                    int mlog_len, const int* __restrict__ start, int mode, int first, int ref, double* __restrict__ out, int cap)
{
	extern __shared__ unsigned short pe_slot[];
	__shared__ double red[4][256];
	const int tid = threadIdx.x, lane = tid & 63;
	const bool timed = mode == 0;
	const int b = blockIdx.x;
	// position j of the path is entry base + j of the log, n positions
	int base = 0, n = L;
	if (timed) n = first + b + 1;
	if (mode == 2) { base = first; n = L - first; }
	if (n < 1 || base + n > L || L > PHD_POSEERR_MAX) return;   // (a whole workgroup; the host launches no such grid)

	// ---- 1. the slots of the path
	if (mode == 2) {
		for (int j = tid; j < n; j += 256) pe_slot[j] = (unsigned short) pe_slot_of(sel, from_marks, mlentry, mlog_len, base + j, P);
	}
	else if (tid < 64) {
		int a = __builtin_amdgcn_readfirstlane(pe_slot_of(sel, from_marks, mlentry, mlog_len, n - 1, P));
		for (int hi = n - 1; hi >= 0; hi -= 64) {
			const int k = hi - lane;
			unsigned long long m = ballot64(k >= 1 && dirty[k] != 0);
			int mine = a;
			while (m) {   // (at most 64 turns: one per bit)
				const int j = __ffsll((long long) m) - 1;
				m &= m - 1;
				a = __builtin_amdgcn_readfirstlane(hist_clamp(parent[(size_t) (hi - j) * Ps + a], P));
				if (lane > j) mine = a;
			}
			if (k >= 0) pe_slot[k] = (unsigned short) mine;
		}
	}
	__syncthreads();

	// ---- 2. the errors
	auto estimate = [&](int j) { return pe_load(pose + ((size_t) (base + j) * Ps + pe_slot[j]) * 7); };
	auto real = [&](int j) { return pe_load(truth + (size_t) (base + j) * 7); };
	const int lo = timed ? start[first + b] : 0;                             // (>= 0: the host counted it)
	const int nodo = 1 + (n > PHD_POSEERR_ODO ? n - PHD_POSEERR_ODO : 0);   // the odometry series: 0.0, then positions 10 .. n - 1
	double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
	for (int j = lo + tid; j < n; j += 256) {
		const int r = j < ref ? j : ref;
		double loc, rot;
		pe_errors(real(j), real(r), estimate(j), estimate(r), &loc, &rot);
		if (timed) { acc0 += loc; acc1 += rot; }
		else { out[j] = loc; out[(size_t) cap + j] = rot; }
	}
	for (int j = (lo > 1 ? lo : 1) + tid; j < nodo; j += 256) {
		const int k = j + PHD_POSEERR_ODO - 1;
		double loc, rot;
		pe_errors(real(k), real(k - PHD_POSEERR_ODO), estimate(k), estimate(k - PHD_POSEERR_ODO), &loc, &rot);
		if (timed) { acc2 += loc; acc3 += rot; }
		else { out[2 * (size_t) cap + j] = loc; out[3 * (size_t) cap + j] = rot; }
	}
	if (!timed) {
		if (tid == 0) { out[2 * (size_t) cap] = 0.0; out[3 * (size_t) cap] = 0.0; }
		return;
	}
	red[0][tid] = acc0; red[1][tid] = acc1; red[2][tid] = acc2; red[3][tid] = acc3;
	__syncthreads();
#pragma unroll
	for (int s = 128; s >= 1; s >>= 1) {
		if (tid < s) {
#pragma unroll
			for (int q = 0; q < 4; q++) red[q][tid] += red[q][tid + s];
		}
		__syncthreads();
	}
	// mean /= localerror.Count - startindex (Plot.cs:356), as written: 0 / 0 is NaN, 0 / a negative count is -0
	if (tid < 4) out[(size_t) tid * cap + b] = red[tid][0] / (double) ((tid < 2 ? n : nodo) - lo);
}
