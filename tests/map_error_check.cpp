// phd_map_error through the C++ host mirror (monorfs_amd/host/PHDNavigator.hpp): three frames with the map log on, then the
// map-error series of the log against a small truth set, with and without an alignment, compared with the host's own metric
// (Loopy.hpp::BestMapEstimate, Ospa.hpp::MapError) on the maps WayMaps returns. Without a HIP device it must fail loudly
// (exit 3); with one it prints the estimate sizes and ends with "map error ok" (exit 0).
#include "../monorfs_amd/host/Loopy.hpp"
#include "../monorfs_amd/host/Ospa.hpp"

#include <cstdio>

int main()
{
	phd_params prm;
	phd_default_params(&prm, 8, 600, 16);
	monorfs::Pose3D pose = {0, 0, 0, 1, 0, 0, 0};
	try {
		monorfs::PHDNavigator nav(prm, pose, 8);
		nav.enableMapHistory(3, 3 * 600);
		std::vector<monorfs::PixelRangeMeasurement> z = {{10, 20, 1.0}, {-50, 30, 0.8}, {100, -60, 1.4}};
		std::vector<std::array<double, 6>> noise(8);
		for (int f = 1; f <= 3; f++) {
			for (int i = 0; i < 8; i++) noise[i] = {1e-4 * (i - 3), 0, -1e-4 * f, 0, 1e-5 * i, 0};
			nav.UpdateOdometry(f / 30.0, {0.01, 0, 0, 0, 0, 0.002}, noise, false);
			nav.SlamUpdate(f / 30.0, z, 0.5);   // (appends: the map log is on)
		}
		const std::vector<std::array<double, 3>> truth = {{0.02, 0.03, 1.0}, {-0.07, 0.04, 0.8}, {0.24, -0.15, 1.4}, {1.0, 1.0, 1.0}};
		const std::array<monorfs::Pose3D, 2> pair = {monorfs::Pose3D{0.01, 0.02, -0.01, 0.999, 0.01, -0.02, 0.03}, monorfs::Pose3D{0, 0.01, 0, 1, 0, 0.01, 0}};
		const std::vector<monorfs::PHDNavigator::WayMap> way = nav.WayMaps();
		if (way.size() != 3) { std::printf("expected 3 entries, got %zu\n", way.size()); return 1; }
		for (int aligned = 0; aligned < 2; aligned++) {
			const double C = aligned ? 0.5 : 1.0, P = aligned ? 2.0 : 1.0;
			std::vector<monorfs::PHDNavigator::MapErrorEntry> got = aligned ? nav.MapError(truth, C, P, {pair, pair, pair}, {1, 0, 1}) : nav.MapError(truth, C, P);
			if (got.size() != 3) { std::printf("expected 3 values, got %zu\n", got.size()); return 1; }
			std::printf(aligned ? "aligned sizes:" : "estimate sizes:");
			for (int f = 0; f < 3; f++) {
				const std::vector<std::array<double, 3>> est = monorfs::BestMapEstimate(way[f].Model);
				double spatial = 0;
				const double ospa = monorfs::MapError(truth, est, aligned && f != 1, pair[0], pair[1], C, P, &spatial);
				std::printf(" %d", got[f].Size);
				if (got[f].Time != (f + 1) / 30.0 || got[f].Size != (int) est.size()) { std::printf("\nentry %d: time or size differs\n", f); return 1; }
				if (std::fabs(got[f].Ospa - ospa) > 1e-12 * C || std::fabs(std::pow(got[f].Spatial, P) - std::pow(spatial, P)) > 1e-12 * std::pow(C, P)) {
					std::printf("\nentry %d: ospa %.17g / %.17g, spatial %.17g / %.17g\n", f, got[f].Ospa, ospa, got[f].Spatial, spatial);
					return 1;
				}
			}
			std::printf("\n");
		}
		std::printf("map error ok\n");
		return 0;
	}
	catch (const monorfs::PhdError& e) {
		std::printf("PhdError status=%d module=%s: %s\n", e.status, e.module.c_str(), e.what());
		return 3;
	}
}
