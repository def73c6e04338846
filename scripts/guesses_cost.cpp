// The C++ host's side of scripts/guesses_cost.py: on frames read from a text file (the format of tests/guesses_check.cpp) times
//   cpp_loop   the guess loop of Loopy.hpp alone (FitToMeasurement, PoseSubtract, the radius test per pair), no device call
//   cpp_stage  monorfs::HostGuesses: that loop and the batch call for the first values
//   cpp_call   PHDNavigator::QuasiGuessesMulti (phd_quasi_guesses_multi)
// and prints {"guesses": n, "ms": {name: [per round]}}. argv: scene file, repeats, warmup.
#include "../monorfs_amd/host/Loopy.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>

static double rd(FILE* f)
{
	double v;
	if (std::fscanf(f, "%lf", &v) != 1) { std::fprintf(stderr, "scene file too short\n"); std::exit(2); }
	return v;
}

static size_t guess_loop(double focal, const std::vector<monorfs::PHDNavigator::QuasiProblem>& problems, const std::vector<monorfs::Odometry>& pose0s,
                         std::vector<std::vector<monorfs::Odometry>>& guesses)
{
	size_t n = 0;
	guesses.assign(problems.size(), {});
	for (size_t i = 0; i < problems.size(); i++) {
		const monorfs::Pose3D initpose = monorfs::PoseAdd(problems[i].LinearPoint, pose0s[i]);
		guesses[i].push_back(pose0s[i]);
		for (const auto& landmark : problems[i].Landmarks) {
			for (const auto& measurement : problems[i].Measurements) {
				const monorfs::Pose3D guess = monorfs::FitToMeasurement(focal, initpose, measurement, landmark);
				const monorfs::Odometry d = monorfs::PoseSubtract(guess, initpose);
				double sq = 0;
				for (double x : d) sq += x * x;
				if (sq < 0.5 * 0.5) guesses[i].push_back(monorfs::PoseSubtract(guess, problems[i].LinearPoint));
			}
		}
		n += guesses[i].size();
	}
	return n;
}

int main(int argc, char** argv)
{
	if (argc < 4) return 2;
	FILE* f = std::fopen(argv[1], "r");
	if (!f) return 2;
	const int repeats = std::atoi(argv[2]), warmup = std::atoi(argv[3]);
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
	phd_default_params(&prm, 4096, 600, 32);
	try {
		monorfs::PHDNavigator nav(prm, problems[0].LinearPoint, 1);
		std::vector<double> loop, stage, call;
		size_t n = 0, nd = 0;
		auto now = [] { return std::chrono::steady_clock::now(); };
		auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
		for (int rep = 0; rep < warmup + repeats; rep++) {
			std::vector<std::vector<monorfs::Odometry>> guesses;
			const auto t0 = now();
			n = guess_loop(prm.measurer[0], problems, pose0s, guesses);
			const auto t1 = now();
			const monorfs::FrameGuesses host = monorfs::HostGuesses(nav, prm.measurer[0], pose0s, problems, 4096);
			const auto t2 = now();
			const monorfs::PHDNavigator::GuessesResult r = nav.QuasiGuessesMulti(problems, pose0s, monorfs::detail::FarPose(), 0.5);
			const auto t3 = now();
			nd = r.Values.size();
			if (rep >= warmup) { loop.push_back(ms(t0, t1)); stage.push_back(ms(t1, t2)); call.push_back(ms(t2, t3)); }
		}
		if (n != nd) { std::fprintf(stderr, "the host loop made %zu guesses, the device %zu\n", n, nd); return 1; }
		std::printf("{\"guesses\": %zu, \"ms\": {", nd);
		const char* names[3] = {"cpp_loop", "cpp_stage", "cpp_call"};
		const std::vector<double>* lists[3] = {&loop, &stage, &call};
		for (int k = 0; k < 3; k++) {
			std::printf("%s\"%s\": [", k ? ", " : "", names[k]);
			for (size_t i = 0; i < lists[k]->size(); i++) std::printf("%s%.4f", i ? ", " : "", (*lists[k])[i]);
			std::printf("]");
		}
		std::printf("}}\n");
	}
	catch (const std::exception& e) {
		std::fprintf(stderr, "%s\n", e.what());
		return 1;
	}
	return 0;
}
