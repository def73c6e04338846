// phd_pose_error through the C++ host mirror (monorfs_amd/host/PHDNavigator.hpp): fourteen frames with both logs on, then the
// pose-error series of the trajectory log against a made-up truth in all three history modes, with the slots given and with
// slots left to the map log, compared with the host's own metric (PoseError.hpp) on the paths WayPointsAt returns.
// Without a HIP device it must fail loudly (exit 3); with one it prints the best slots and ends with "pose error ok" (exit 0).
#include "../monorfs_amd/host/PoseError.hpp"

#include <cmath>
#include <cstdio>

using namespace monorfs;

static bool close(const std::vector<double>& got, const std::vector<double>& gott, const TimedValue& want, double tol, const char* what, int mode)
{
	if (got.size() != want.size() || gott.size() != want.size()) { std::printf("mode %d, %s: %zu values, expected %zu\n", mode, what, got.size(), want.size()); return false; }
	for (size_t k = 0; k < want.size(); k++) {
		const double a = got[k], b = want[k].second;
		const bool same = std::isnan(b) ? std::isnan(a) : (b == 0.0 && std::signbit(b)) ? (a == 0.0 && std::signbit(a)) : std::fabs(a - b) <= tol;
		if (!same || gott[k] != want[k].first) { std::printf("mode %d, %s[%zu]: %.17g at %g, expected %.17g at %g\n", mode, what, k, a, gott[k], b, want[k].first); return false; }
	}
	return true;
}

int main()
{
	const int P = 8, FRAMES = 14;
	phd_params prm;
	phd_default_params(&prm, P, 600, 16);
	Pose3D pose = {0, 0, 0, 1, 0, 0, 0};
	try {
		PHDNavigator nav(prm, pose, P);
		nav.enableHistory(FRAMES + 1);
		nav.enableMapHistory(FRAMES, FRAMES * 600);
		nav.appendHistory(0.0);   // entry 0: the constructor's waypoint, no frame's
		std::vector<PixelRangeMeasurement> z = {{10, 20, 1.0}, {-50, 30, 0.8}, {100, -60, 1.4}};
		std::vector<std::array<double, 6>> noise(P);
		for (int f = 1; f <= FRAMES; f++) {
			for (int i = 0; i < P; i++) noise[i] = {1e-3 * (i - 3), 2e-4 * i * f, -1e-3 * f, 1e-3 * i, 2e-3 * (i % 3), -1e-3 * f};
			nav.UpdateOdometry(f / 30.0, {0.01, 0, 0.002, 0, 0.001, 0.02}, noise, false);   // (appends: the log is on)
			nav.SlamUpdate(f / 30.0, z, 0.5);                                                // (appends: the map log is on)
		}
		const int L = FRAMES + 1;
		// the estimate at entry k: the best of the newest map entry appended before it, slot 0 if none
		const std::vector<PHDNavigator::WayMap> way = nav.WayMaps();
		std::vector<int32_t> slots(L, 0);
		for (int k = 2; k < L; k++) slots[k] = way[k - 2].Best;
		std::printf("best slots:");
		for (int k = 0; k < L; k++) std::printf(" %d", slots[k]);
		std::printf("\n");
		// the truth: a smooth path of its own, 1e-2 and more away from any estimate in location and in rotation
		std::vector<Pose3D> truth(L);
		TimedState G(L);
		double S = 1;
		for (int k = 0; k < L; k++) {
			const double a = 0.05 + 0.03 * k;
			truth[k] = Pose3D{0.012 * k, 0.02 * std::sin(0.5 * k), 0.004 * k, 2 * std::cos(a / 2), 2 * std::sin(a / 2), 0, 0};   // (norm 2: FromState scales it)
			G[k] = {k / 30.0, truth[k]};
		}
		const int first = 1;
		TimedTrajectory estimate;
		for (int i = first; i < L; i++) {
			const PHDNavigator::Trajectories t = nav.WayPointsAt(i, {slots[i]});
			TimedState path(i + 1);
			for (int k = 0; k <= i; k++) {
				path[k] = {t.Times[k], t.Poses[0][k]};
				for (int c = 0; c < 3; c++) S = std::max(S, 1 + std::fabs(path[k].second[c]));
			}
			estimate.push_back({t.Times[i], path});
		}
		// The rotation bound comes from these inputs' conditioning, not from a fixed ceiling: an angle is 2 acos(w) of a quaternion
		// that a chain of a few dozen products, two norms and a log / exp pair has rounded (the log's own acos is undone by the exp:
		// no loss there), allowed 64 ulp here; the acos turns an error e of w into 2 e / sin(angle / 2). With `least` the smallest
		// per-pose angle that is not identically 0 (Smooth and Filter state them one by one; Timed's means move by no more):
		// 128 * 2^-52 / sin(least / 2), which must stay under the 1e-9 that tests/test_gpu_pose_error.py takes for a ceiling.
		const double slam = 3.5 / 30.0;
		double least = INFINITY;
		for (int mode = 1; mode < 3; mode++) {
			for (int ref : {0, 4}) {
				const PoseErrors want = PoseError((HistMode) mode, G, estimate, ref, slam);
				for (const TimedValue* series : {&want.Rotation, &want.OdoRotation})
					for (const auto& v : *series) if (v.second != 0) least = std::min(least, v.second);
			}
		}
		const double rottol = 128 * std::ldexp(1.0, -52) / std::sin(least / 2);
		std::printf("smallest per-pose rotation error: %.3g; the device is allowed %.3g\n", least, rottol);
		if (!(least > 0) || !(rottol <= 1e-9)) { std::printf("the truth is too close to an estimate for a comparison of angles\n"); return 1; }
		double worst = 0;
		for (int mode = 0; mode < 3; mode++) {
			for (int ref : {0, 4}) {
				const PoseErrors want = PoseError((HistMode) mode, G, estimate, ref, slam);
				for (int given = 0; given < 2; given++) {
					const PHDNavigator::PoseErrorSeries got = nav.PoseError(truth, mode, given ? slots : std::vector<int32_t>(), first, ref, slam);
					// (a location as in tests/test_gpu_pose_error.py: 1e-12 S)
					if (!close(got.Location, got.Times, want.Location, 1e-12 * S, "location", mode) || !close(got.Rotation, got.Times, want.Rotation, rottol, "rotation", mode) ||
					    !close(got.OdoLocation, got.OdoTimes, want.OdoLocation, 1e-12 * S, "odometry location", mode) ||
					    !close(got.OdoRotation, got.OdoTimes, want.OdoRotation, rottol, "odometry rotation", mode))
						return 1;
					for (size_t k = 0; k < want.Rotation.size(); k++) if (!std::isnan(want.Rotation[k].second)) worst = std::max(worst, std::fabs(got.Rotation[k] - want.Rotation[k].second));
					for (size_t k = 0; k < want.OdoRotation.size(); k++) if (!std::isnan(want.OdoRotation[k].second)) worst = std::max(worst, std::fabs(got.OdoRotation[k] - want.OdoRotation[k].second));
				}
			}
		}
		std::printf("largest rotation difference: %.3g\n", worst);
		std::printf("pose error ok\n");
		return 0;
	}
	catch (const PhdError& e) {
		std::printf("PhdError status=%d module=%s: %s\n", e.status, e.module.c_str(), e.what());
		return 3;
	}
}
