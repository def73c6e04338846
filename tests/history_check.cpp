// The trajectory log through the C++ host mirror (monorfs_amd/host/PHDNavigator.hpp): three frames with the log on, then the
// best particle's path. Without a HIP device it must fail loudly (exit 3); with one it ends with "history ok" (exit 0).
#include "../monorfs_amd/host/PHDNavigator.hpp"

#include <cmath>
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
		std::vector<monorfs::PixelRangeMeasurement> z = {{10, 20, 1.0}, {-50, 30, 0.8}, {100, -60, 1.4}};
		std::vector<std::array<double, 6>> noise(8);
		for (int f = 1; f <= 3; f++) {
			for (int i = 0; i < 8; i++) noise[i] = {1e-4 * (i - 3), 0, -1e-4 * f, 0, 1e-5 * i, 0};
			nav.UpdateOdometry(f / 30.0, {0.01, 0, 0, 0, 0, 0.002}, noise, false);
			nav.SlamUpdate(z, 0.5);
		}
		const int best = nav.BestParticle();
		monorfs::PHDNavigator::Trajectories w = nav.WayPoints({best});
		if (w.Times.size() != 4 || w.Poses.size() != 1 || w.Poses[0].size() != 4) { std::printf("expected a path of 4 entries, got %zu\n", w.Times.size()); return 1; }
		if (w.Times[3] != 3 / 30.0 || w.Poses[0][0] != pose) { std::printf("the path does not start at the reset pose / end at the last frame's time\n"); return 1; }
		const monorfs::Pose3D last = w.Poses[0][3], now = nav.VehicleParticles()[best];
		if (last != now) { std::printf("the last waypoint is not the best particle's pose\n"); return 1; }
		bool full = false;
		try { nav.appendHistory(1.0); }
		catch (const monorfs::PhdError& e) { full = e.status == PHD_ERR_CAPACITY; }
		if (!full) { std::printf("a fifth entry in a log of four was not refused with PHD_ERR_CAPACITY\n"); return 1; }
		std::printf("best particle %d: path of %zu entries, last pose %.6f %.6f %.6f | %.6f %.6f %.6f %.6f (slot %d)\n", best, w.Poses[0].size(),
		            last[0], last[1], last[2], last[3], last[4], last[5], last[6], w.Slots[0][3]);
		std::printf("history ok\n");
		return 0;
	}
	catch (const monorfs::PhdError& e) {
		std::printf("PhdError status=%d module=%s: %s\n", e.status, e.module.c_str(), e.what());
		return 3;
	}
}
