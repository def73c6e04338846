// The map log through the C++ host mirror (monorfs_amd/host/PHDNavigator.hpp): three frames with both logs on, then the best
// map of every frame and the best particle's path as of the last frame's Update. Without a HIP device it must fail loudly
// (exit 3); with one it prints the best map sizes and ends with "map history ok" (exit 0).
#include "../monorfs_amd/host/PHDNavigator.hpp"

#include <cstdio>

int main()
{
	phd_params prm;
	phd_default_params(&prm, 8, 600, 16);
	monorfs::Pose3D pose = {0, 0, 0, 1, 0, 0, 0};
	try {
		monorfs::PHDNavigator nav(prm, pose, 8);
		nav.enableHistory(4);
		nav.appendHistory(0.0);   // Vehicle's constructor (Vehicle.cs:228)
		nav.enableMapHistory(3, 3 * 600);
		std::vector<monorfs::PixelRangeMeasurement> z = {{10, 20, 1.0}, {-50, 30, 0.8}, {100, -60, 1.4}};
		std::vector<std::array<double, 6>> noise(8);
		std::vector<monorfs::Map> maps;
		std::vector<int> best;
		std::vector<monorfs::Pose3D> poses;
		for (int f = 1; f <= 3; f++) {
			for (int i = 0; i < 8; i++) noise[i] = {1e-4 * (i - 3), 0, -1e-4 * f, 0, 1e-5 * i, 0};
			nav.UpdateOdometry(f / 30.0, {0.01, 0, 0, 0, 0, 0.002}, noise, false);
			nav.SlamUpdate(f / 30.0, z, 0.5);   // (appends: the map log is on)
			best.push_back(nav.BestParticle());
			maps.push_back(nav.BestMapModel());
			poses.push_back(nav.BestEstimate());
		}
		const std::vector<monorfs::PHDNavigator::WayMap> way = nav.WayMaps();
		if (way.size() != 3) { std::printf("expected 3 entries, got %zu\n", way.size()); return 1; }
		std::printf("best map sizes:");
		for (int f = 0; f < 3; f++) {
			const monorfs::PHDNavigator::WayMap& e = way[f];
			std::printf(" %zu", e.Model.size());
			if (e.Time != (f + 1) / 30.0 || e.Best != best[f] || e.Pose != poses[f] || e.Model.size() != maps[f].size()) { std::printf("\nentry %d differs from what the getters gave behind that step\n", f); return 1; }
			for (size_t i = 0; i < maps[f].size(); i++) {
				if (e.Model[i].weight != maps[f][i].weight || e.Model[i].mean != maps[f][i].mean || e.Model[i].covariance != maps[f][i].covariance) { std::printf("\nentry %d, component %zu differs\n", f, i); return 1; }
			}
		}
		std::printf("\n");
		if (way[2].Model.empty()) { std::printf("the last best map is empty\n"); return 1; }
		// the path UpdateTrajectory would have copied at the last frame's Update: the best particle then is entry 1's
		monorfs::PHDNavigator::Trajectories w = nav.WayPointsAt(3, {way[1].Best});
		if (w.Times.size() != 4 || w.Poses[0].size() != 4 || w.Slots[0][3] != way[1].Best || w.Poses[0][0] != pose) { std::printf("the path as of entry 3 is not 4 entries from the reset pose\n"); return 1; }
		bool full = false;
		try { nav.appendMapHistory(1.0); }
		catch (const monorfs::PhdError& e) { full = e.status == PHD_ERR_CAPACITY; }
		if (!full) { std::printf("a fourth entry in a log of three was not refused with PHD_ERR_CAPACITY\n"); return 1; }
		std::printf("map history ok\n");
		return 0;
	}
	catch (const monorfs::PhdError& e) {
		std::printf("PhdError status=%d module=%s: %s\n", e.status, e.module.c_str(), e.what());
		return 3;
	}
}
