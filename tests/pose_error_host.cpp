// monorfs_amd/host/PoseError.hpp alone, without a device or the library: a stand-alone program for the tests (and for a
// sanitizer build: g++ -fsanitize=address,undefined tests/pose_error_host.cpp).
//
//   pose_error_host cases     the hand-checkable cases below; prints one line per case, ends with "cases ok" (exit 0), or names
//                             the first assertion that does not hold (exit 1)
//   pose_error_host series    reads doubles (native binary) from stdin: L, nq; times[L]; truth[L][7]; for i = 0 .. L - 1 the
//                             estimated path as of entry i, [i + 1][7]; nq queries of (mode, first_entry, ref_entry, slam_time).
//                             Prints per query "query q", "clock <ms of the metric> ms", then per series "series <name> <n>" and
//                             n lines "time value" (%.17g).
#include "../monorfs_amd/host/PoseError.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>

using namespace monorfs;

static Pose3D turned_z(double x, double y, double z, double angle) { return Pose3D{x, y, z, std::cos(angle / 2), 0, 0, std::sin(angle / 2)}; }

static detail::Q quat(const Pose3D& p) { return detail::Q{p[3], p[4], p[5], p[6]}; }

#define EXPECT(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n  ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

static TimedTrajectory prefixes(const TimedState& path, int first)
{
	TimedTrajectory e;
	for (size_t i = first; i < path.size(); i++) e.push_back({path[i].first, TimedState(path.begin(), path.begin() + i + 1)});
	return e;
}

static int cases()
{
	// a truth path that starts at the identity orientation, moves in the plane and turns about z
	TimedState G;
	for (int k = 0; k < 14; k++) G.push_back({k / 30.0, turned_z(0.1 * k, 0.03 * k * k, 0.02 * k, 0.07 * k)});

	{   // 1. estimate = truth: all four series are 0 (the rotation one within 1e-7: acos at 1)
		for (int mode = 0; mode < 3; mode++) {
			const PoseErrors e = PoseError((HistMode) mode, G, prefixes(G, 0), 3, 0.0);
			for (const TimedValue* s : {&e.Location, &e.Rotation, &e.OdoLocation, &e.OdoRotation}) {
				for (const auto& v : *s) EXPECT(std::fabs(v.second) <= (s == &e.Rotation || s == &e.OdoRotation ? 1e-7 : 1e-14), "mode %d: %.17g at t = %g", mode, v.second, v.first);
			}
			EXPECT(e.Location.size() == 14 && e.OdoLocation.size() == (mode == 0 ? 14u : 5u), "lengths %zu, %zu", e.Location.size(), e.OdoLocation.size());
		}
		std::printf("case estimate equals truth: zero\n");
	}
	{   // 2. a constant rigid offset at every entry: the location moved by c, the orientation turned by theta about z in the
		//    world frame (q_c q). With ref_entry = 0 and G[0] at the identity orientation, the relative location of the estimate is
		//    R_c^T (G[k] - G[0]) against G[k] - G[0]: the error is 2 sin(theta / 2) |(G[k] - G[0])_xy|, 0 at entry 0; no rotation error
		const double theta = 0.4, c[3] = {0.5, -0.2, 0.1};
		const detail::Q qc{std::cos(theta / 2), 0, 0, std::sin(theta / 2)};
		TimedState E;
		for (const auto& g : G) {
			const detail::Q q = detail::qmul(qc, quat(g.second));
			E.push_back({g.first, Pose3D{g.second[0] + c[0], g.second[1] + c[1], g.second[2] + c[2], q.w, q.x, q.y, q.z}});
		}
		const TimedValue loc = LocationError0(G, E, 0), rot = RotationError0(G, E, 0);
		EXPECT(loc[0].second == 0.0, "entry 0: %.17g", loc[0].second);
		for (int k = 1; k < 14; k++) {
			const double want = 2 * std::sin(theta / 2) * std::hypot(G[k].second[0] - G[0].second[0], G[k].second[1] - G[0].second[1]);
			EXPECT(std::fabs(loc[k].second - want) <= 1e-12 * (1 + want), "entry %d: %.17g, closed form %.17g", k, loc[k].second, want);
			EXPECT(std::fabs(rot[k].second) <= 1e-7, "entry %d: rotation %.17g", k, rot[k].second);
		}
		std::printf("case rigid offset: closed form\n");
	}
	for (double theta : {0.01, 1.0, 3.0}) {   // 3. the orientation turned by theta about one (body) axis at every k > ref_entry: rotation error theta
		const int ref = 2;
		const detail::Q qt{std::cos(theta / 2), 0, std::sin(theta / 2), 0};
		TimedState E = G;
		for (int k = ref + 1; k < 14; k++) {
			const detail::Q q = detail::qmul(quat(G[k].second), qt);
			E[k].second = Pose3D{G[k].second[0], G[k].second[1], G[k].second[2], q.w, q.x, q.y, q.z};
		}
		const TimedValue rot = RotationError0(G, E, ref), loc = LocationError0(G, E, ref);
		for (int k = 0; k < 14; k++) {
			const double want = k > ref ? theta : 0.0;
			EXPECT(std::fabs(rot[k].second - want) <= 1e-9, "theta %g, entry %d: %.17g", theta, k, rot[k].second);
			EXPECT(std::fabs(loc[k].second) <= 1e-12, "theta %g, entry %d: location %.17g", theta, k, loc[k].second);
		}
		// (the odometry series compares k with k - 10: the same where k - 10 <= ref, the entries that are not turned)
		const TimedValue odo = OdoRotationError0(G, E);
		for (size_t j = 1; j < odo.size() && (int) j + 9 - 10 <= ref; j++) {
			EXPECT(std::fabs(odo[j].second - theta) <= 1e-9, "theta %g, odometry entry %zu: %.17g", theta, j, odo[j].second);
		}
		std::printf("case turned by %g: rotation error %g\n", theta, theta);
	}
	{   // 4. the odometry series of a path shorter than 11: the constant alone; 11 poses: one value more, at the time of entry 10
		for (int n = 1; n <= 11; n++) {
			const TimedState g(G.begin(), G.begin() + n);
			TimedState e = g;
			for (auto& p : e) p.second[0] += 0.01 * p.first * 30;
			const TimedValue a = OdoLocationError0(g, e), b = OdoRotationError0(g, e);
			EXPECT(a.size() == (n < 11 ? 1u : 2u) && b.size() == a.size(), "%d poses: %zu values", n, a.size());
			EXPECT(a[0].second == 0.0 && b[0].second == 0.0 && a[0].first == G[0].first, "%d poses: entry 0 is %.17g at %g", n, a[0].second, a[0].first);
			if (n == 11) EXPECT(a[1].first == G[10].first && std::fabs(a[1].second - 0.1) <= 1e-12, "11 poses: %.17g at %g", a[1].second, a[1].first);
		}
		std::printf("case short odometry series: the constant alone\n");
	}
	{   // 5. the Timed division with slam_time behind every entry: start_i = i. The odometry series of estimate i has
		//    n = 1 + max(0, i + 1 - 10) values: i = 0 gives 0 / 1, i = 1 gives 0 / 0 = NaN, i >= 2 gives 0 / (n - i) = -0
		TimedState E = G;
		for (auto& p : E) p.second[1] += 0.05;
		E[0] = G[0];
		const PoseErrors t = PoseError(HistMode::Timed, G, prefixes(E, 0), 0, 100.0);
		EXPECT(t.OdoLocation.size() == 14 && t.Location.size() == 14, "lengths");
		EXPECT(t.OdoLocation[0].second == 0.0 && !std::signbit(t.OdoLocation[0].second), "estimate 0: %.17g", t.OdoLocation[0].second);
		EXPECT(std::isnan(t.OdoLocation[1].second) && std::isnan(t.OdoRotation[1].second), "estimate 1 is not the NaN of 0 / 0: %.17g", t.OdoLocation[1].second);
		for (int i = 2; i < 14; i++) {
			EXPECT(t.OdoLocation[i].second == 0.0 && std::signbit(t.OdoLocation[i].second), "estimate %d is not the -0 of 0 / negative: %.17g", i, t.OdoLocation[i].second);
			EXPECT(t.OdoRotation[i].second == 0.0 && std::signbit(t.OdoRotation[i].second), "estimate %d (rotation) is not -0: %.17g", i, t.OdoRotation[i].second);
		}
		// ... and the location mean of estimate i is its newest pose's error alone: 0.05, the offset relative to entry 0
		for (int i = 1; i < 14; i++) EXPECT(std::fabs(t.Location[i].second - 0.05) <= 1e-12, "estimate %d: %.17g", i, t.Location[i].second);
		// slam_time inside the record: start stops growing behind it
		const PoseErrors u = PoseError(HistMode::Timed, G, prefixes(E, 0), 0, 2.5 / 30.0);
		EXPECT(std::fabs(u.Location[13].second - 0.05) <= 1e-12 && std::fabs(u.OdoLocation[13].second) <= 1e-12, "slam_time inside: %.17g %.17g",
		       u.Location[13].second, u.OdoLocation[13].second);
		std::printf("case timed division: NaN and -0\n");
	}
	std::printf("cases ok\n");
	return 0;
}

static bool take(double* to, size_t n) { return std::fread(to, sizeof(double), n, stdin) == n; }

static int series()
{
	double head[2];
	if (!take(head, 2)) return 2;
	const int L = (int) head[0], nq = (int) head[1];
	if (L < 1 || nq < 0) return 2;
	std::vector<double> times(L), row(7);
	if (!take(times.data(), L)) return 2;
	TimedState G(L);
	for (int k = 0; k < L; k++) {
		if (!take(G[k].second.data(), 7)) return 2;
		G[k].first = times[k];
	}
	TimedTrajectory all(L);
	for (int i = 0; i < L; i++) {
		all[i].first = times[i];
		all[i].second.resize(i + 1);
		for (int k = 0; k <= i; k++) {
			if (!take(all[i].second[k].second.data(), 7)) return 2;
			all[i].second[k].first = times[k];
		}
	}
	for (int q = 0; q < nq; q++) {
		double query[4];
		if (!take(query, 4)) return 2;
		const int mode = (int) query[0], first = (int) query[1], ref = (int) query[2];
		if (mode < 0 || mode > 2 || first < 0 || first >= L || ref < 0) return 2;
		const TimedTrajectory estimate(all.begin() + first, all.end());
		const auto t0 = std::chrono::steady_clock::now();
		const PoseErrors e = PoseError((HistMode) mode, G, estimate, ref, query[3]);
		const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		std::printf("query %d\nclock %.3f ms\n", q, ms);
		const char* names[4] = {"location", "rotation", "odolocation", "odorotation"};
		const TimedValue* s[4] = {&e.Location, &e.Rotation, &e.OdoLocation, &e.OdoRotation};
		for (int i = 0; i < 4; i++) {
			std::printf("series %s %zu\n", names[i], s[i]->size());
			for (const auto& v : *s[i]) std::printf("%.17g %.17g\n", v.first, v.second);
		}
	}
	return 0;
}

int main(int argc, char** argv)
{
	if (argc == 2 && !std::strcmp(argv[1], "cases")) return cases();
	if (argc == 2 && !std::strcmp(argv[1], "series")) return series();
	std::printf("usage: pose_error_host cases | series < input\n");
	return 2;
}
