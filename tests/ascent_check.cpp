// Runs the resident ascent of the C++ host mirror (monorfs_amd/host/Loopy.hpp: LogLikeGradientAscent and FitGaussian with
// resident = true, over PHDNavigator::QuasiAscent) on a scene read from a text file and prints the results with 17 digits;
// tests/test_gpu_ascent.py compares them with PHDNavigator.QuasiAscent of the Python host.
// scene file: "J M n" then J landmarks (3), M measurements (3), linearpoint (7), n initial estimates (6).
#include "../monorfs_amd/host/Loopy.hpp"

#include <cstdio>
#include <cstdlib>

static double rd(FILE* f)
{
	double v;
	if (std::fscanf(f, "%lf", &v) != 1) { std::fprintf(stderr, "scene file too short\n"); std::exit(2); }
	return v;
}

int main(int argc, char** argv)
{
	if (argc < 3) return 2;
	FILE* f = std::fopen(argv[1], "r");
	if (!f) return 2;
	const int mode = std::atoi(argv[2]);
	const int J = (int) rd(f), M = (int) rd(f), n = (int) rd(f);
	std::vector<std::array<double, 3>> lm(J);
	std::vector<monorfs::PixelRangeMeasurement> z(M);
	for (auto& l : lm) for (double& x : l) x = rd(f);
	for (auto& m : z) for (double& x : m) x = rd(f);
	monorfs::Pose3D lin;
	for (double& x : lin) x = rd(f);
	std::vector<monorfs::Odometry> starts(n);
	for (auto& s : starts) for (double& x : s) x = rd(f);
	std::fclose(f);

	phd_params prm;
	phd_default_params(&prm, 256, 600, 16);
	try {
		monorfs::PHDNavigator nav(prm, lin, 1);
		std::vector<double> loglike;
		std::vector<monorfs::Odometry> poses = monorfs::LogLikeGradientAscent(nav, starts, z, lm, lin, loglike, 256, mode, 1e-2, 10, true);
		for (int a = 0; a < n; a++) {
			std::printf("ascent %.17g", loglike[a]);
			for (double x : poses[a]) std::printf(" %.17g", x);
			std::printf("\n");
		}
		// the bound: one iteration, the state at the bound
		poses = monorfs::LogLikeGradientAscent(nav, starts, z, lm, lin, loglike, 256, mode, 1e-2, 10, true, 1);
		for (int a = 0; a < n; a++) {
			std::printf("bounded %.17g", loglike[a]);
			for (double x : poses[a]) std::printf(" %.17g", x);
			std::printf("\n");
		}
		std::pair<monorfs::Odometry, monorfs::Matrix6> fit = monorfs::FitGaussian(nav, starts[0], z, lm, lin, 256, mode, true);
		std::printf("fitmean");
		for (double x : fit.first) std::printf(" %.17g", x);
		std::printf("\nfitcovariance");
		for (double x : fit.second) std::printf(" %.17g", x);
		std::printf("\n");
	}
	catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
	return 0;
}
