// PHDNavigator.hpp — C++ host-side mirror of the reference's solver interface over libphdhip.so.
//
// The reference's host is C# (no .NET toolchain in this image), so the native host written here is
// C++: the class keeps the member names, argument meaning and error behaviour of
//     class PHDNavigator<PRM3DMeasurer, Pose3D, PixelRangeMeasurement> : Navigator<...>
//     (mono-rfs-lib/SLAM/Navigators/PHDNavigator.cs:52-983; Navigator.cs:47-396)
// and forwards each member to the C-ABI of include/phdhip.h. Nothing is computed here.
//
// Errors: a non-zero status becomes a PhdError whose `module` is "association" for
// PHD_ERR_ASSOCIATION — what Simulation.Update looks for in Data["module"] (Simulation.cs:655-670).
#pragma once
#include "../../include/phdhip.h"

#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace monorfs {

struct PhdError : std::runtime_error {
	int         status;
	std::string module;
	PhdError(int status, const std::string& what)
		: std::runtime_error(what), status(status), module(status == PHD_ERR_ASSOCIATION ? "association" : "phdhip") {}
};

// one Gaussian component of a Map (BaseStructures/Gaussian.cs:49-59)
struct Gaussian {
	double weight;
	std::array<double, 3> mean;
	std::array<double, 9> covariance;   // row-major
};
typedef std::vector<Gaussian> Map;       // BaseStructures/Maps/Map.cs, canonical (insertion) order
typedef std::array<double, 7> Pose3D;    // x y z qw qx qy qz (Pose3D.cs:142-162)
typedef std::array<double, 3> PixelRangeMeasurement;   // px py range

class PHDNavigator {
public:
	// ≙ PHDNavigator(vehicle, particlecount, onlymapping) (PHDNavigator.cs:192-208)
	PHDNavigator(const phd_params& params, const Pose3D& pose, int particlecount, bool onlymapping = false, int device = 0)
		: ParticleCount(particlecount), OnlyMapping(onlymapping)
	{
		nav_ = phd_create(&params, device);
		if (!nav_) throw PhdError(PHD_ERR_NO_DEVICE, phd_create_error());
		reset(pose, Map(), onlymapping ? 1 : particlecount);   // :201-207
	}
	// the particles sharded over several GPUs of the node behind one handle (phd_create_multi): params.max_particles and
	// particlecount are totals, multiples of devices.size()
	PHDNavigator(const phd_params& params, const Pose3D& pose, int particlecount, const std::vector<int>& devices, bool onlymapping = false)
		: ParticleCount(particlecount), OnlyMapping(onlymapping)
	{
		nav_ = phd_create_multi(&params, devices.data(), (int) devices.size());
		if (!nav_) throw PhdError(PHD_ERR_NO_DEVICE, phd_create_error());
		reset(pose, Map(), particlecount);
	}
	~PHDNavigator() { Dispose(); }
	PHDNavigator(const PHDNavigator&) = delete;
	PHDNavigator& operator=(const PHDNavigator&) = delete;

	void Dispose()   // Navigator.cs:395
	{
		if (nav_) phd_destroy(nav_);
		nav_ = nullptr;
	}

	int  ParticleCount;   // :118
	bool OnlyMapping;     // Navigator.cs:129

	// ≙ Update (:295-314): the motion model (TrackVehicle.UpdateNoisy) and its RNG stay on the host
	void Update(const std::vector<Pose3D>& particleposes)
	{
		check(phd_set_poses(nav_, particleposes.empty() ? nullptr : particleposes[0].data(), (int) particleposes.size()));
	}

	// The same step with the motion model on the device (phd_update_motion): the odometry reading and
	// one noise vector per particle (dt * chol(MotionCovariance) * N(0, I), drawn by the host; empty: none)
	void UpdateOdometry(const std::array<double, 6>& reading, const std::vector<std::array<double, 6>>& noise, bool perfectstill)
	{
		check(phd_update_motion(nav_, reading.data(), noise.empty() ? nullptr : noise[0].data(), ParticleCount, perfectstill ? 1 : 0));
	}
	// ... with the frame's time: the same, and its waypoint when the trajectory log is on (Vehicle.Update, Vehicle.cs:335)
	void UpdateOdometry(double time, const std::array<double, 6>& reading, const std::vector<std::array<double, 6>>& noise, bool perfectstill)
	{
		UpdateOdometry(reading, noise, perfectstill);
		if (history_) appendHistory(time);
	}

	// The particles' paths on the device (phd_history_enable): room for `capacity` entries, 0 switches the log off; every
	// call restarts it at length 0 (ResetHistory)
	void enableHistory(int capacity)
	{
		check(phd_history_enable(nav_, capacity));
		history_ = capacity > 0;
	}

	// one entry: the current particle poses (phd_history_append; asynchronous)
	void appendHistory(double time) { check(phd_history_append(nav_, time)); }

	// ≙ VehicleParticles[i].WayPoints (Vehicle.cs:141) of the listed particles of the current state, oldest entry first
	// (phd_trajectories; waits for the device): Times[L], Poses[n][L], Slots[n][L] — the slot the ancestor held at that entry
	struct Trajectories {
		std::vector<double> Times;
		std::vector<std::vector<Pose3D>> Poses;
		std::vector<std::vector<int32_t>> Slots;
	};
	Trajectories WayPoints(const std::vector<int32_t>& particles)
	{
		int L = 0;
		const double *t = nullptr, *x = nullptr;
		const int32_t* s = nullptr;
		check(phd_trajectories(nav_, particles.data(), (int) particles.size(), &L, &t, &x, &s));
		return trajectories(particles.size(), L, t, x, s);
	}

	// WayPoints as they were at trajectory-log entry `entry`, of the particles that held `slots` then: entry + 1 entries, nothing
	// that resampled later enters (phd_trajectories_at; waits for the device)
	Trajectories WayPointsAt(int entry, const std::vector<int32_t>& slots)
	{
		int L = 0;
		const double *t = nullptr, *x = nullptr;
		const int32_t* s = nullptr;
		check(phd_trajectories_at(nav_, entry, slots.data(), (int) slots.size(), &L, &t, &x, &s));
		return trajectories(slots.size(), L, t, x, s);
	}

	// The best map of every frame on the device (phd_map_history_enable; Navigator.WayMaps): room for `entries` entries and
	// `components` components over all of them, entries = 0 switches the log off; every call restarts it
	void enableMapHistory(int entries, int64_t components)
	{
		check(phd_map_history_enable(nav_, entries, components));
		maphistory_ = entries > 0;
	}

	// one entry: the best particle's map, slot and pose (phd_map_history_append; asynchronous)
	void appendMapHistory(double time) { check(phd_map_history_append(nav_, time)); }

	// ≙ Navigator.WayMaps (Navigator.cs:269-272) with the best particle beside every map, oldest entry first (phd_map_history;
	// waits for the device). An entry whose components did not fit the log throws (PHD_ERR_CAPACITY).
	struct WayMap {
		double  Time;
		int32_t Best;
		Pose3D  Pose;
		Map     Model;
	};
	std::vector<WayMap> WayMaps()
	{
		int L = 0;
		const double *t = nullptr, *x = nullptr, *w = nullptr, *m = nullptr, *c = nullptr;
		const int32_t *b = nullptr, *n = nullptr;
		const int64_t* off = nullptr;
		check(phd_map_history(nav_, &L, &t, &b, &x, &n, &off, &w, &m, &c));
		std::vector<WayMap> out(L);
		for (int k = 0; k < L; k++) {
			out[k].Time = t[k];
			out[k].Best = b[k];
			std::copy(x + k * 7, x + k * 7 + 7, out[k].Pose.begin());
			out[k].Model = tomap(n[k], w + off[k], m + off[k] * 3, c + off[k] * 9);
		}
		return out;
	}

	// ≙ Plot.MapError (postanalysis/Plot.cs:478-529) over the map log, on the device (phd_map_error; waits for it): for every
	// entry the OSPA distance with cut-off C and order P between `truth` (the visited map) and Map.BestMapEstimate of the logged
	// map, its cardinality and spatial parts and the estimate's size. align: empty, or per entry the estimated and the true pose
	// at the reference time; hasreference: empty (every entry is aligned) or per entry. Ospa.hpp is the same metric on the host.
	struct MapErrorEntry {
		double  Time, Ospa, Cardinality, Spatial;
		int32_t Size;
	};
	std::vector<MapErrorEntry> MapError(const std::vector<std::array<double, 3>>& truth, double C = 1.0, double P = 1.0,
	                                    const std::vector<std::array<Pose3D, 2>>& align = {}, const std::vector<uint8_t>& hasreference = {})
	{
		int L = 0;
		const double *t = nullptr, *o = nullptr, *c = nullptr, *s = nullptr;
		const int32_t* n = nullptr;
		check(phd_map_error(nav_, truth.empty() ? nullptr : truth[0].data(), (int) truth.size(), C, P, align.empty() ? nullptr : align[0][0].data(),
		                    hasreference.empty() ? nullptr : hasreference.data(), &L, &t, &o, &c, &s, &n));
		std::vector<MapErrorEntry> out(L);
		for (int k = 0; k < L; k++) out[k] = {t[k], o[k], c[k], s[k], n[k]};
		return out;
	}

	// ≙ Plot.LocationError / RotationError / OdoLocationError / OdoRotationError (postanalysis/Plot.cs:293-456) over the
	// trajectory log, on the device (phd_pose_error; waits for it). truth: the true pose at every entry of the log. mode:
	// PHD_POSE_ERROR_TIMED / _SMOOTH / _FILTER. slots: per entry the slot whose path is the estimate then; empty: the best
	// particle of the map log. The estimates are the entries from first_entry on; ref_entry is the entry both paths are taken
	// relative to (Plot.RefTime); slam_time the time of the "SLAM ... on" tag, 0 without one. PoseError.hpp is the same metric
	// on the host.
	struct PoseErrorSeries {
		std::vector<double> Times, Location, Rotation, OdoTimes, OdoLocation, OdoRotation;
	};
	PoseErrorSeries PoseError(const std::vector<Pose3D>& truth, int mode = PHD_POSE_ERROR_TIMED, const std::vector<int32_t>& slots = {},
	                          int first_entry = 0, int ref_entry = 0, double slam_time = 0.0)
	{
		if (!slots.empty() && slots.size() != truth.size()) throw std::invalid_argument("PoseError: one slot per true pose");
		int n = 0, m = 0;
		const double *t = nullptr, *a = nullptr, *r = nullptr, *ot = nullptr, *oa = nullptr, *orot = nullptr;
		check(phd_pose_error(nav_, mode, truth.empty() ? nullptr : truth[0].data(), (int) truth.size(), slots.empty() ? nullptr : slots.data(),
		                     first_entry, ref_entry, slam_time, &n, &t, &a, &r, &m, &ot, &oa, &orot));
		PoseErrorSeries out;
		out.Times.assign(t, t + n); out.Location.assign(a, a + n); out.Rotation.assign(r, r + n);
		out.OdoTimes.assign(ot, ot + m); out.OdoLocation.assign(oa, oa + m); out.OdoRotation.assign(orot, orot + m);
		return out;
	}

	// ≙ static QuasiSetLogLikelihood(measurements, map, pose) (:526-531), for a batch of candidate poses (row f4)
	std::vector<double> QuasiSetLogLikelihood(const std::vector<PixelRangeMeasurement>& measurements,
	                                          const std::vector<std::array<double, 3>>& landmarks, const std::vector<Pose3D>& poses)
	{
		std::vector<double> out(poses.size());
		check(phd_quasi_set_loglik(nav_, poses.empty() ? nullptr : poses[0].data(), (int) poses.size(),
		                           landmarks.empty() ? nullptr : landmarks[0].data(), (int) landmarks.size(),
		                           measurements.empty() ? nullptr : measurements[0].data(), (int) measurements.size(), out.data()));
		return out;
	}

	// ≙ static QuasiSetLogLikelihood(measurements, map, pose, out gradient) (:543-548) for a batch of candidate poses;
	// averagemode: TemperedAverage as its source reads (0) or with weights that sum to one (1), see phdhip.h
	std::vector<double> QuasiSetLogLikelihood(const std::vector<PixelRangeMeasurement>& measurements,
	                                          const std::vector<std::array<double, 3>>& landmarks, const std::vector<Pose3D>& poses,
	                                          std::vector<std::array<double, 6>>& gradients, int averagemode = 0)
	{
		std::vector<double> out(poses.size());
		gradients.assign(poses.size(), std::array<double, 6>{});
		check(phd_quasi_set_loglik_grad(nav_, poses.empty() ? nullptr : poses[0].data(), (int) poses.size(),
		                                landmarks.empty() ? nullptr : landmarks[0].data(), (int) landmarks.size(),
		                                measurements.empty() ? nullptr : measurements[0].data(), (int) measurements.size(), averagemode,
		                                out.data(), gradients.empty() ? nullptr : gradients[0].data()));
		return out;
	}

	// ≙ LoopyPHDNavigator.LogLikeGradientAscent (LoopyPHDNavigator.cs:916-965) for the initial estimates side by side, resident on
	// the device (phd_quasi_ascent): one call per maxestimates estimates (<= the handle's max_particles / PHD_ASCENT_LINE).
	// Capped: an estimate was still climbing after maxiterations iterations (PHD_ERR_CAPACITY; its state at the bound is
	// returned). Hessians (withhessians): the raw finite-difference rows of LogLikeFitCovariance at the returned poses.
	struct AscentResult {
		std::vector<std::array<double, 6>>  Poses;
		std::vector<double>                 Values;
		std::vector<int32_t>                Iterations;
		std::vector<std::array<double, 36>> Hessians;
		bool                                Capped = false;
	};
	AscentResult QuasiAscent(const std::vector<std::array<double, 6>>& initial, const std::vector<PixelRangeMeasurement>& measurements,
	                         const std::vector<std::array<double, 3>>& landmarks, const Pose3D& linearpoint, int maxestimates,
	                         int averagemode = 0, int maxiterations = 1000, int rounditerations = 0, bool withhessians = false)
	{
		const size_t n = initial.size(), chunk = (size_t) (maxestimates > 0 ? maxestimates : 1);
		AscentResult out;
		out.Poses.resize(n); out.Values.resize(n); out.Iterations.resize(n);
		if (withhessians) out.Hessians.resize(n);
		for (size_t s = 0; s < n; s += chunk) {
			const int m = (int) std::min(chunk, n - s);
			const int rc = phd_quasi_ascent(nav_, initial[s].data(), m, linearpoint.data(), landmarks.empty() ? nullptr : landmarks[0].data(),
			                                (int) landmarks.size(), measurements.empty() ? nullptr : measurements[0].data(), (int) measurements.size(),
			                                averagemode, maxiterations, rounditerations, out.Poses[s].data(), &out.Values[s], &out.Iterations[s],
			                                withhessians ? out.Hessians[s].data() : nullptr);
			if (rc == PHD_ERR_CAPACITY) out.Capped = true;
			else check(rc);
		}
		return out;
	}

	// What differs between the frames of LoopyPHDNavigator.UpdateMessagesFromMap (:525-551): a problem of the calls below
	struct QuasiProblem {
		std::vector<std::array<double, 3>> Landmarks;
		std::vector<PixelRangeMeasurement> Measurements;
		Pose3D                             LinearPoint{0, 0, 0, 1, 0, 0, 0};
	};

	// QuasiAscent for the estimates of many problems in the same launches (phd_quasi_ascent_multi): estimate e starts at
	// initial[e] and is searched against problems[problem[e]]; every estimate bit for bit as from QuasiAscent with its problem
	// alone. A C call takes problems of one measurement-block class (<= 64, 65..128, 129..256 measurements) and maxestimates
	// estimates: the estimates are split by class and chunked, the results come back in the caller's order.
	AscentResult QuasiAscentMulti(const std::vector<QuasiProblem>& problems, const std::vector<std::array<double, 6>>& initial,
	                              const std::vector<int>& problem, int maxestimates, int averagemode = 0, int maxiterations = 1000,
	                              int rounditerations = 0, bool withhessians = false)
	{
		const size_t n = initial.size();
		checkProblems(problems, problem, n);
		AscentResult out;
		out.Poses.resize(n); out.Values.resize(n); out.Iterations.resize(n);
		if (withhessians) out.Hessians.resize(n);
		for (const std::vector<int>& idx : multiCalls(problems, problem, maxestimates)) {
			const PackedProblems pk = packProblems(problems, problem, idx, true);
			const size_t k = idx.size();
			std::vector<std::array<double, 6>> start(k), poses(k);
			std::vector<double> values(k);
			std::vector<int32_t> iterations(k);
			std::vector<std::array<double, 36>> hessians(withhessians ? k : 0);
			for (size_t j = 0; j < k; j++) start[j] = initial[idx[j]];
			const int rc = phd_quasi_ascent_multi(nav_, (int) pk.lmoff.size() - 1, pk.lmoff.data(), pk.lm.empty() ? nullptr : pk.lm[0].data(),
			                                      pk.zoff.data(), pk.z.empty() ? nullptr : pk.z[0].data(), pk.lin[0].data(), start[0].data(),
			                                      pk.which.data(), (int) k, averagemode, maxiterations, rounditerations, poses[0].data(),
			                                      values.data(), iterations.data(), withhessians ? hessians[0].data() : nullptr);
			if (rc == PHD_ERR_CAPACITY) out.Capped = true;
			else check(rc);
			for (size_t j = 0; j < k; j++) {
				out.Poses[idx[j]] = poses[j]; out.Values[idx[j]] = values[j]; out.Iterations[idx[j]] = iterations[j];
				if (withhessians) out.Hessians[idx[j]] = hessians[j];
			}
		}
		return out;
	}

	// QuasiSetLogLikelihood for poses of many problems in one launch (phd_quasi_set_loglik_multi): pose i against
	// problems[problem[i]], at most maxposes (<= the handle's max_particles) a call
	std::vector<double> QuasiSetLogLikelihoodMulti(const std::vector<QuasiProblem>& problems, const std::vector<Pose3D>& poses,
	                                               const std::vector<int>& problem, int maxposes)
	{
		return quasiBatchMulti(problems, poses, problem, maxposes, 0, nullptr);
	}

	// ... with the gradients (phd_quasi_set_loglik_multi with gradients6)
	std::vector<double> QuasiSetLogLikelihoodGradientMulti(const std::vector<QuasiProblem>& problems, const std::vector<Pose3D>& poses,
	                                                       const std::vector<int>& problem, std::vector<std::array<double, 6>>& gradients,
	                                                       int maxposes, int averagemode = 0)
	{
		gradients.assign(poses.size(), std::array<double, 6>{});
		return quasiBatchMulti(problems, poses, problem, maxposes, averagemode, &gradients);
	}

	// The starting guesses of GuidedFitMixture (LoopyPHDNavigator.cs:789-797) for many problems and their first values
	// (phd_quasi_guesses_multi): the guesses of problem q stand at Offsets[q] .. Offsets[q + 1], pose0s[q] first (pair -1, -1), then
	// the (landmark, measurement) pairs whose fitted pose lies within `radius` of the initial pose, landmark-major. Poses =
	// LinearPoint.Add(guess), Values = QuasiSetLogLikelihood there, EmptySpace[q] = the value of `farpose` against problem q.
	struct GuessesResult {
		std::vector<int32_t>                Offsets;      // [problems + 1]
		std::vector<std::array<int32_t, 2>> Pairs;
		std::vector<std::array<double, 6>>  Guesses;
		std::vector<Pose3D>                 Poses;
		std::vector<double>                 Values, EmptySpace;
	};

	// The problems are split by measurement-block class; a call that reports more guesses than its arrays hold is repeated once
	// with the reported total; the results come back in the caller's order.
	GuessesResult QuasiGuessesMulti(const std::vector<QuasiProblem>& problems, const std::vector<std::array<double, 6>>& pose0s,
	                                const Pose3D& farpose, double radius = 0.5)
	{
		const size_t T = problems.size();
		if (pose0s.size() != T) throw std::invalid_argument("one initial pose per problem");
		std::vector<int> all(T);
		for (size_t q = 0; q < T; q++) all[q] = (int) q;
		struct Part { std::vector<int32_t> off; std::vector<std::array<int32_t, 2>> pairs; std::vector<std::array<double, 6>> guesses; std::vector<Pose3D> poses; std::vector<double> values; };
		std::vector<Part> parts;
		std::vector<std::pair<int, int>> where(T);   // problem q: (part, index within it)
		GuessesResult out;
		out.EmptySpace.assign(T, 0.0);
		for (const std::vector<int>& idx : multiCalls(problems, all, (int) std::max<size_t>(T, 1))) {
			const PackedProblems pk = packProblems(problems, all, idx, true);   // (idx is ascending: the problems in that order)
			const size_t k = idx.size();
			std::vector<std::array<double, 6>> start(k);
			size_t pairs = 0;
			for (size_t j = 0; j < k; j++) { start[j] = pose0s[idx[j]]; pairs += problems[idx[j]].Landmarks.size() * problems[idx[j]].Measurements.size(); }
			Part p;
			p.off.assign(k + 1, 0);
			std::vector<double> empty(k);
			int capacity = (int) (k + std::min(pairs, 64 * k));   // (every pair, or a first try of 64 a problem)
			int rc = PHD_OK;
			for (int attempt = 0; attempt < 2; attempt++) {
				const size_t room = (size_t) std::max(capacity, 1);
				p.pairs.assign(room, {0, 0}); p.guesses.assign(room, {}); p.poses.assign(room, Pose3D{}); p.values.assign(room, 0.0);
				rc = phd_quasi_guesses_multi(nav_, (int) k, pk.lmoff.data(), pk.lm.empty() ? nullptr : pk.lm[0].data(), pk.zoff.data(),
				                             pk.z.empty() ? nullptr : pk.z[0].data(), pk.lin[0].data(), start[0].data(), farpose.data(), radius, capacity,
				                             p.off.data(), p.pairs[0].data(), p.guesses[0].data(), p.poses[0].data(), p.values.data(), empty.data());
				if (rc != PHD_ERR_CAPACITY) break;
				capacity = p.off[k];   // (guess_offsets is set: the total the retry needs)
			}
			check(rc);
			for (size_t j = 0; j < k; j++) { where[idx[j]] = {(int) parts.size(), (int) j}; out.EmptySpace[idx[j]] = empty[j]; }
			parts.push_back(std::move(p));
		}
		out.Offsets.assign(T + 1, 0);
		for (size_t q = 0; q < T; q++) {
			const Part& p = parts[where[q].first];
			const int32_t a = p.off[where[q].second], b = p.off[where[q].second + 1];
			out.Offsets[q + 1] = out.Offsets[q] + (b - a);
			out.Pairs.insert(out.Pairs.end(), p.pairs.begin() + a, p.pairs.begin() + b);
			out.Guesses.insert(out.Guesses.end(), p.guesses.begin() + a, p.guesses.begin() + b);
			out.Poses.insert(out.Poses.end(), p.poses.begin() + a, p.poses.begin() + b);
			out.Values.insert(out.Values.end(), p.values.begin() + a, p.values.begin() + b);
		}
		return out;
	}

	// KinectMeasurer's current depth frame (phd_set_depth_map): `depth` row-major [height][width] (the reference's
	// float[ResX][ResY] frame transposed), used by every step until the next call; an empty vector switches it off
	void setDepthMap(const std::vector<float>& depth, int width, int height)
	{
		check(depth.empty() ? phd_set_depth_map(nav_, nullptr, 0, 0) : phd_set_depth_map(nav_, depth.data(), width, height));
	}

	// ≙ SlamUpdate (:323-362); `uniform` replaces (double) Util.Uniform.Next() of ResampleParticles (:727)
	void SlamUpdate(const std::vector<PixelRangeMeasurement>& measurements, double uniform)
	{
		check(phd_slam_update(nav_, measurements.empty() ? nullptr : measurements[0].data(), (int) measurements.size(),
		                      OnlyMapping ? 1 : 0, uniform));
	}
	// ... with the frame's time: the same, and the best map's entry when the map log is on (UpdateMapHistory, :361)
	void SlamUpdate(double time, const std::vector<PixelRangeMeasurement>& measurements, double uniform)
	{
		SlamUpdate(measurements, uniform);
		if (maphistory_) appendMapHistory(time);
	}

	// The step in its asynchronous parts (phd_set_measurements / phd_sync), and one mapping-only step that particle slot `held`
	// sits out: behind it the slot has the mixture it had in front of it, bit for bit; -1 holds nobody (phd_step_hold_async).
	// StepHold posts the step and returns; what a posted step finds surfaces at Sync.
	void SetMeasurements(const std::vector<PixelRangeMeasurement>& measurements)
	{
		check(phd_set_measurements(nav_, measurements.empty() ? nullptr : measurements[0].data(), (int) measurements.size()));
	}
	void StepHold(int held) { check(phd_step_hold_async(nav_, held)); }
	void Sync() { check(phd_sync(nav_)); }

	std::vector<double> VehicleWeights()   // :128
	{
		int n = 0;
		const double* w = phd_weights(nav_, &n);
		if (!w) throw PhdError(PHD_ERR_DEVICE, phd_last_error(nav_));
		return std::vector<double>(w, w + n);
	}

	int BestParticle() { return phd_best_particle(nav_); }   // :139

	std::vector<Pose3D> VehicleParticles()   // poses of :123
	{
		int n = 0;
		const double* p = phd_poses(nav_, &n);
		if (!p) throw PhdError(PHD_ERR_DEVICE, phd_last_error(nav_));
		std::vector<Pose3D> out(n / 7);
		for (int i = 0; i < n / 7; i++) std::copy(p + i * 7, p + i * 7 + 7, out[i].begin());
		return out;
	}

	Pose3D BestEstimate() { return VehicleParticles()[BestParticle()]; }   // :144-150

	Map MapModels(int particle)   // :134
	{
		int n = 0;
		const double *w, *m, *c;
		check(phd_map(nav_, particle, &n, &w, &m, &c));
		return tomap(n, w, m, c);
	}

	Map BestMapModel() { return MapModels(BestParticle()); }   // :155-161

	// ≙ reset (:245-266)
	void reset(const Pose3D& pose, const Map& model, int particlecount)
	{
		std::vector<double> w, m, c;
		frommap(model, w, m, c);
		check(phd_reset(nav_, particlecount, pose.data(), w.data(), m.data(), c.data(), (int) model.size()));
	}

	void CollapseParticles(int particlecount) { reset(BestEstimate(), BestMapModel(), particlecount); }   // :233-236
	void StartSlamInternal() { CollapseParticles(ParticleCount); }                                        // :214-217
	void StartMappingInternal() { CollapseParticles(1); }                                                 // :224-227

	void ResetMapModel()   // :271-276
	{
		int P = phd_particle_count(nav_);
		for (int i = 0; i < P; i++) check(phd_set_map(nav_, i, nullptr, nullptr, nullptr, 0));
	}

	// ≙ ResampleParticles (:724-760) / ParticleDepleted (:768-777) on given weights
	std::vector<int32_t> ResampleParticles(const std::vector<double>& weights, double uniform, int* best = nullptr)
	{
		std::vector<int32_t> src(weights.size());
		int32_t b = 0;
		check(phd_resample(nav_, weights.data(), (int) weights.size(), uniform, src.data(), &b));
		if (best) *best = b;
		return src;
	}

	bool ParticleDepleted(const std::vector<double>& weights)
	{
		uint8_t d = 0;
		check(phd_particle_depleted(nav_, weights.data(), (int) weights.size(), &d));
		return d != 0;
	}

	// after a SlamUpdate: the slot every particle was copied from (identity if no resampling), so the
	// host can permute what it keeps per particle (trajectories, TrackVehicle objects)
	std::vector<int32_t> ResampleSources(bool* resampled = nullptr)
	{
		int n = 0;
		uint8_t r = 0;
		const int32_t* s = phd_resample_sources(nav_, &n, &r);
		if (!s) throw PhdError(PHD_ERR_DEVICE, phd_last_error(nav_));
		if (resampled) *resampled = r != 0;
		return std::vector<int32_t>(s, s + n);
	}

	phd_navigator* handle() { return nav_; }

private:
	void check(int status)
	{
		if (status != PHD_OK) throw PhdError(status, phd_last_error(nav_));
	}

	// ---- the calls over many problems: which items go into which C call, and a call's problem table
	struct PackedProblems {
		std::vector<int32_t>               lmoff, zoff, which;   // offsets of the problems a call names; its items' problems, renumbered
		std::vector<std::array<double, 3>> lm, z;                // the pools
		std::vector<Pose3D>                lin;
	};

	static int blockClass(size_t m) { return m == 0 ? 0 : (m <= 64 ? 1 : (m <= 128 ? 2 : 4)); }   // 0: fits any class

	static void checkProblems(const std::vector<QuasiProblem>& problems, const std::vector<int>& problem, size_t n)
	{
		bool ok = problem.size() == n;
		for (int q : problem) ok = ok && q >= 0 && (size_t) q < problems.size();
		if (!ok) throw std::invalid_argument("one problem index in [0, problems.size()) per estimate or pose");
	}

	// lists of item indices, each of one block class and at most percall long, the caller's order kept within a call; the items of
	// problems without measurements ride with the first class that has any
	static std::vector<std::vector<int>> multiCalls(const std::vector<QuasiProblem>& problems, const std::vector<int>& problem, int percall)
	{
		const size_t chunk = (size_t) (percall > 0 ? percall : 1);
		int first = 0;
		for (int cls : {4, 2, 1}) for (int q : problem) if (blockClass(problems[q].Measurements.size()) == cls) first = cls;
		if (!first) first = 1;
		std::vector<std::vector<int>> calls;
		for (int cls : {1, 2, 4}) {
			std::vector<int> idx;
			for (size_t i = 0; i < problem.size(); i++) {
				const int c = blockClass(problems[problem[i]].Measurements.size());
				if ((c ? c : first) == cls) idx.push_back((int) i);
			}
			for (size_t s = 0; s < idx.size(); s += chunk) calls.emplace_back(idx.begin() + s, idx.begin() + std::min(idx.size(), s + chunk));
		}
		return calls;
	}

	static PackedProblems packProblems(const std::vector<QuasiProblem>& problems, const std::vector<int>& problem, const std::vector<int>& idx, bool withlin)
	{
		PackedProblems pk;
		std::vector<int> renum(problems.size(), -1);
		std::vector<int> used;
		for (int i : idx) if (renum[problem[i]] < 0) { renum[problem[i]] = 0; used.push_back(problem[i]); }
		std::sort(used.begin(), used.end());
		pk.lmoff.push_back(0); pk.zoff.push_back(0);
		for (size_t k = 0; k < used.size(); k++) {
			const QuasiProblem& p = problems[used[k]];
			renum[used[k]] = (int) k;
			pk.lm.insert(pk.lm.end(), p.Landmarks.begin(), p.Landmarks.end());
			pk.z.insert(pk.z.end(), p.Measurements.begin(), p.Measurements.end());
			pk.lmoff.push_back((int32_t) pk.lm.size()); pk.zoff.push_back((int32_t) pk.z.size());
			if (withlin) pk.lin.push_back(p.LinearPoint);
		}
		for (int i : idx) pk.which.push_back(renum[problem[i]]);
		return pk;
	}

	std::vector<double> quasiBatchMulti(const std::vector<QuasiProblem>& problems, const std::vector<Pose3D>& poses, const std::vector<int>& problem,
	                                    int maxposes, int averagemode, std::vector<std::array<double, 6>>* gradients)
	{
		checkProblems(problems, problem, poses.size());
		std::vector<double> out(poses.size());
		for (const std::vector<int>& idx : multiCalls(problems, problem, maxposes)) {
			const PackedProblems pk = packProblems(problems, problem, idx, false);
			const size_t k = idx.size();
			std::vector<Pose3D> at(k);
			std::vector<double> values(k);
			std::vector<std::array<double, 6>> grad(gradients ? k : 0);
			for (size_t j = 0; j < k; j++) at[j] = poses[idx[j]];
			check(phd_quasi_set_loglik_multi(nav_, (int) pk.lmoff.size() - 1, pk.lmoff.data(), pk.lm.empty() ? nullptr : pk.lm[0].data(),
			                                 pk.zoff.data(), pk.z.empty() ? nullptr : pk.z[0].data(), at[0].data(), pk.which.data(), (int) k,
			                                 averagemode, values.data(), gradients ? grad[0].data() : nullptr));
			for (size_t j = 0; j < k; j++) {
				out[idx[j]] = values[j];
				if (gradients) (*gradients)[idx[j]] = grad[j];
			}
		}
		return out;
	}

	static Trajectories trajectories(size_t n, int L, const double* t, const double* x, const int32_t* s)
	{
		Trajectories out;
		out.Times.assign(t, t + (L > 0 ? L : 0));
		out.Poses.assign(n, std::vector<Pose3D>(L));
		out.Slots.assign(n, std::vector<int32_t>(L));
		for (size_t j = 0; j < n; j++) {
			for (int k = 0; k < L; k++) {
				const double* q = x + (j * L + k) * 7;
				std::copy(q, q + 7, out.Poses[j][k].begin());
				out.Slots[j][k] = s[j * L + k];
			}
		}
		return out;
	}

	static Map tomap(int n, const double* w, const double* m, const double* c)
	{
		Map out(n);
		for (int i = 0; i < n; i++) {
			out[i].weight = w[i];
			std::copy(m + i * 3, m + i * 3 + 3, out[i].mean.begin());
			std::copy(c + i * 9, c + i * 9 + 9, out[i].covariance.begin());
		}
		return out;
	}

	static void frommap(const Map& map, std::vector<double>& w, std::vector<double>& m, std::vector<double>& c)
	{
		w.assign(map.size() + 1, 0);
		m.assign(map.size() * 3 + 3, 0);
		c.assign(map.size() * 9 + 9, 0);
		for (size_t i = 0; i < map.size(); i++) {
			w[i] = map[i].weight;
			std::copy(map[i].mean.begin(), map[i].mean.end(), m.begin() + i * 3);
			std::copy(map[i].covariance.begin(), map[i].covariance.end(), c.begin() + i * 9);
		}
	}

	phd_navigator* nav_ = nullptr;
	bool history_ = false;   // the trajectory log is on: UpdateOdometry(time, ...) appends
	bool maphistory_ = false;   // the map log is on: SlamUpdate(time, ...) appends
};

}  // namespace monorfs
