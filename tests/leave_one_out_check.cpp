// Runs Loopy.hpp::LeaveOneOutMaps of the C++ host mirror on a scene read from a text file and prints every map with 17 digits;
// tests/test_leave_one_out_host_cpp.py compares them with monorfs_amd/loopy.py. Without a HIP device it must fail loudly (exit 3).
// scene file: "T maxparticles" then T frames of (time, pose 7, count, count measurements (3)).
#include "../monorfs_amd/host/Loopy.hpp"

#include <cstdio>
#include <cstdlib>

static double rd(FILE* f)
{
	double v;
	if (std::fscanf(f, "%lf", &v) != 1) { std::fprintf(stderr, "scene file too short\n"); std::exit(2); }
	return v;
}

static void print(const char* what, int index, const monorfs::Map& map)
{
	std::printf("%s %d %zu\n", what, index, map.size());
	for (const monorfs::Gaussian& c : map) {
		std::printf("component %.17g", c.weight);
		for (double x : c.mean) std::printf(" %.17g", x);
		for (double x : c.covariance) std::printf(" %.17g", x);
		std::printf("\n");
	}
}

int main(int argc, char** argv)
{
	if (argc < 2) return 2;
	FILE* f = std::fopen(argv[1], "r");
	if (!f) return 2;
	const int T = (int) rd(f), maxparticles = (int) rd(f);
	std::vector<std::pair<double, monorfs::Pose3D>> trajectory(T);
	std::vector<std::pair<double, std::vector<monorfs::PixelRangeMeasurement>>> factors(T);
	for (int t = 0; t < T; t++) {
		trajectory[t].first = factors[t].first = rd(f);
		for (double& x : trajectory[t].second) x = rd(f);
		factors[t].second.resize((int) rd(f));
		for (auto& m : factors[t].second) for (double& x : m) x = rd(f);
	}
	std::fclose(f);

	phd_params prm;
	phd_default_params(&prm, maxparticles, 600, 16);
	try {
		monorfs::PHDNavigator nav(prm, T > 0 ? trajectory[0].second : monorfs::Pose3D{0, 0, 0, 1, 0, 0, 0}, 1);
		monorfs::Map full;
		const std::vector<monorfs::Map> maps = monorfs::LeaveOneOutMaps(nav, trajectory, factors, maxparticles, &full);
		for (size_t i = 0; i < maps.size(); i++) print("map", (int) i, maps[i]);
		print("full", -1, full);
		// an index outside the frames leaves nothing out; a duplicate gives the same map twice
		const std::vector<monorfs::Map> some = monorfs::LeaveOneOutMaps(nav, trajectory, factors, {1, 1, -1, T + 3}, T, maxparticles);
		for (size_t i = 0; i < some.size(); i++) print("some", (int) i, some[i]);
		std::printf("leave one out ok\n");
		return 0;
	}
	catch (const monorfs::PhdError& e) {
		std::printf("PhdError status=%d module=%s: %s\n", e.status, e.module.c_str(), e.what());
		return 3;
	}
}
