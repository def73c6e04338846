// Runs the guess stage of the C++ host mirror (monorfs_amd/host/PHDNavigator.hpp: QuasiGuessesMulti; monorfs_amd/host/Loopy.hpp:
// HostGuesses, GuidedFitMixtures(..., device_guesses)) on problems read from a text file and prints the results with 17 digits;
// tests/test_gpu_guesses.py compares them with the Python host.
// scene file: "P", then per problem "J M", J landmarks (3), M measurements (3), linearpoint (7), pose0 (6). The fits run against
// a map of weight 1.0001 per landmark.
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
	const int P = (int) rd(f);
	std::vector<monorfs::PHDNavigator::QuasiProblem> problems(P);
	std::vector<monorfs::Odometry> pose0s(P);
	for (int q = 0; q < P; q++) {
		auto& p = problems[q];
		const int J = (int) rd(f), M = (int) rd(f);
		p.Landmarks.resize(J);
		p.Measurements.resize(M);
		for (auto& l : p.Landmarks) for (double& x : l) x = rd(f);
		for (auto& m : p.Measurements) for (double& x : m) x = rd(f);
		for (double& x : p.LinearPoint) x = rd(f);
		for (double& x : pose0s[q]) x = rd(f);
	}
	std::fclose(f);

	phd_params prm;
	phd_default_params(&prm, 256, 600, 16);
	try {
		monorfs::PHDNavigator nav(prm, problems[0].LinearPoint, 1);
		const monorfs::PHDNavigator::GuessesResult r = nav.QuasiGuessesMulti(problems, pose0s, monorfs::detail::FarPose(), 0.5);
		std::printf("offsets");
		for (int32_t o : r.Offsets) std::printf(" %d", (int) o);
		std::printf("\n");
		for (size_t e = 0; e < r.Values.size(); e++) {
			std::printf("guess %d %d", (int) r.Pairs[e][0], (int) r.Pairs[e][1]);
			for (double x : r.Guesses[e]) std::printf(" %.17g", x);
			for (double x : r.Poses[e]) std::printf(" %.17g", x);
			std::printf(" %.17g\n", r.Values[e]);
		}
		for (int q = 0; q < P; q++) std::printf("empty %d %.17g\n", q, r.EmptySpace[q]);
		const monorfs::FrameGuesses host = monorfs::HostGuesses(nav, prm.measurer[0], pose0s, problems, 256);
		for (int q = 0; q < P; q++) {
			for (size_t e = 0; e < host.Guesses[q].size(); e++) {
				std::printf("hostguess %d %d %d", q, host.Pairs[q][e][0], host.Pairs[q][e][1]);
				for (double x : host.Guesses[q][e]) std::printf(" %.17g", x);
				std::printf("\n");
			}
		}
		std::vector<std::vector<monorfs::PixelRangeMeasurement>> zs;
		std::vector<monorfs::Map> maps;
		std::vector<monorfs::Pose3D> lins;
		for (const auto& p : problems) {
			monorfs::Map map;
			for (const auto& l : p.Landmarks) map.push_back(monorfs::Gaussian{1.0001, l, {1e-4, 0, 0, 0, 1e-4, 0, 0, 0, 1e-4}});
			zs.push_back(p.Measurements); maps.push_back(map); lins.push_back(p.LinearPoint);
		}
		std::vector<double> empties;
		const std::vector<std::vector<monorfs::PoseComponent>> fits = monorfs::GuidedFitMixtures(nav, prm.measurer[0], pose0s, zs, maps, lins, 256, &empties, mode, 0, true);
		for (int k = 0; k < P; k++) {
			std::printf("fit %d %d %.17g\n", k, (int) fits[k].size(), empties[k]);
			for (size_t j = 0; j < fits[k].size(); j++) {
				std::printf("fitmean %d %d", k, (int) j);
				for (double x : fits[k][j].mean) std::printf(" %.17g", x);
				std::printf("\n");
			}
		}
	}
	catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
	return 0;
}
