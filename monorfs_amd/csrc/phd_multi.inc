// phd_multi.inc — the multi-device handle of phd_create_multi (included by phdhip.hip).
//
// SURVEY §8b asks for a device list behind the C-ABI: the reference drives its solver from ONE managed thread
// (Simulation.Update, Simulation.cs:636-673; binding precedent ISAM2Navigator.cs:600-622), and a C# host has no RCCL. A
// multi-device handle therefore owns one shard handle per device (particles sharded contiguously, SURVEY §8e) and plays
// the sharded step itself. The caller's thread only POSTS a step; one worker thread per shard issues it on that shard's
// device and stream, so the host cost of a step does not grow with the number of devices and phd_step_async returns at
// once. Nothing in a step waits for the host:
//   local step on every shard (the devices run concurrently); its last kernel stores the shard's un-normalised weights
//     straight into every shard's gathered vector through peer-mapped pointers (the all-gather of SURVEY §5 / §8e: 16 KB
//     of stores per peer over xGMI at 2048 particles per GPU), together with the shard's status word
//   every shard waits, ON ITS STREAM, for the other shards' stores (one event per shard and step)
//   the identical global normalise / BestParticle / depletion test / systematic resampling on every shard, then the
//     migration plan, on the device (k_plan_migration)
//   migration of the particles whose source lives on another shard: the sender packs each record straight into its place
//     in the receiver's buffer (peer stores again), the receiver waits for the senders' events and unpacks
// — the kernels a process-per-GPU host drives with RCCL (bench.py), with peer stores in place of the collectives.
// Results are bit-identical to a single handle holding all particles, for any number of devices (tests/test_gpu_multi.py).
//
// Ordering between shards (nothing but stream order and the two events per shard and step):
//   * shard t's weights of step k land in shard s's vector before s's global kernel of step k: s's stream waits for
//     ev_gather[t] of step k;
//   * they do not land while s's global / plan / scatter kernels of step k - 1 still read it: t stores them behind its own
//     finish kernel of step k - 1, which waited for ev_pack[s] of step k - 1, recorded behind those kernels;
//   * shard s's records of step k land in t's receive buffer before t's finish kernel of step k (ev_pack[s]) and not while
//     t's finish kernel of step k - 1 still reads it: s packs behind its global kernel of step k, which waited for
//     ev_gather[t] of step k, recorded behind t's finish kernel of step k - 1.
// A worker must not make its stream wait for an event before the owner has recorded it for this step (the wait would
// take the previous record): the per-shard step counters gather_rec / pack_rec say when; events alternate between two sets
// so that a record of step k + 1 can never be mistaken for that of step k.
//
// Visibility between DEVICES (what makes a peer store of shard t readable by a later kernel of shard s, beyond the order above):
//   * the buffers other devices store into — every shard's gathered weight vector d_gw and receive buffer d_recv — are
//     FINE-GRAINED device memory (hipExtMallocWithFlags(hipDeviceMallocFinegrained); ensure_sharded / ensure_gw): the
//     allocation class that is coherent between agents, which is what RCCL allocates for its own peer-to-peer buffers. The
//     owning device does not keep such lines in its L2 across the peers' writes, so a later kernel cannot read a stale copy of
//     a line a peer has rewritten; the storing device does not hold the remote lines back in its L2 either. (When the
//     runtime refuses the flag the buffers are ordinary allocations — phd_migration_recv_is_finegrained says so — and the
//     argument falls back on the kernel boundaries alone, below.)
//   * release: t's stores are issued by k_push_weights / k_pack_particles; the hipEventRecord behind the kernel completes only
//     when the kernel has — the end of a kernel is a release of everything its waves stored, at system scope for the
//     dispatches HIP issues in front of an event another device's stream will wait for (the events are created with
//     hipEventDisableTiming only, i.e. with the default system-scope release: no hipEventReleaseToDevice);
//   * acquire: s's stream waits for that event (hipStreamWaitEvent on ANOTHER device's event is a barrier packet on s's queue),
//     and the kernel dispatched behind it starts with an acquire: its waves' first loads of d_gw / d_recv go to memory.
//   * the process-per-GPU host (bench.py --gpus N) relies on the same two halves with RCCL in the middle: the pushing kernel
//     ends (release), the one-word all-reduce on the same stream cannot complete on ANY rank before every rank's push kernel
//     has ended (its own kernel is stream-ordered behind the push on every rank), and k_finish_sharded is a new dispatch behind
//     it (acquire). The receive buffers there are the same fine-grained allocations, opened through hipIpcMemHandle.
// Not run on two distinct devices by the builder (one-GPU boxes): the tests cover the ordering with all shards on device 0 and,
// across PROCESSES, the IPC path (tests/test_gpu_multiproc.py).

#define MULTI_RING 256
#define MULTI_PH_SAMPLES 64

struct MultiCmd { uint8_t onlymapping; double u; };

struct MultiState {
	std::vector<phd_navigator*> sh;     // shard handles, shard s holds particles [s * Pl, (s + 1) * Pl)
	std::vector<int> devices;
	std::vector<hipEvent_t> ev_gather[2], ev_pack[2];
	std::vector<uint8_t> p2p;           // [n][n] 1: shard s reaches shard t's memory directly (peer access, or the same device)
	int n = 0;
	int Pl = 0;                         // particles per shard
	int shard_cap = 0;                  // ... it can hold
	std::vector<double> h_weights, h_poses;
	std::vector<int32_t> h_src;
	int M = 0;
	// the workers
	std::vector<std::thread> workers;
	std::mutex mu;
	std::condition_variable cv_work;
	MultiCmd ring[MULTI_RING];
	std::atomic<long long> posted{0};
	std::unique_ptr<std::atomic<long long>[]> issued, gather_rec, pack_rec;   // per shard: steps issued / events recorded
	std::atomic<int> stop{0}, failed{0};
	int fail_code = PHD_OK, fail_shard = 0;
	std::string fail_msg;
	// diagnostics (phd_multi_report)
	double post_us = 0; long long posts = 0;                   // the caller's thread inside phd_step_async
	std::unique_ptr<double[]> issue_us, spin_us; long long issue_steps = 0;   // per shard: its worker's time issuing steps; of it, waiting for the other workers' records
	bool ph_on = false; int ph_period = 1, ph_count = 0;
	hipEvent_t ph_ev[MULTI_PH_SAMPLES][6];                     // phase boundaries of sampled steps, on shard 0's stream
	bool ph_made = false;
};

static int multi_fail_from(phd_navigator* nav, phd_navigator* shard, int rc, int s)
{
	return nav->fail(rc, "device " + std::to_string(shard->device) + " (shard " + std::to_string(s) + "): " + shard->err);
}

phd_navigator* multi_shard0(phd_navigator* nav);

static inline void cpu_pause() { __builtin_ia32_pause(); }

// A worker waits for another worker's step counter: a short spin (the other thread is normally a few microseconds behind),
// then yields and sleeps — with fewer cores than shards, or a CPU quota, a spinning thread must not starve the one it waits
// for — and gives up after a minute: a worker stuck inside a HIP call then marks the handle failed instead of hanging
// phd_sync / phd_destroy for ever. Returns false on the timeout.
static bool multi_wait_counter(const std::atomic<long long>& c, long long target)
{
	for (int spins = 0; c.load(std::memory_order_acquire) < target; spins++) {
		if (spins < 2000) cpu_pause();
		else if (spins < 4000) std::this_thread::yield();
		else {
			std::this_thread::sleep_for(std::chrono::microseconds(50));
			if (spins > 4000 + 1200000) return false;   // ~ 60 s
		}
	}
	return true;
}

// Every step posted so far has been ISSUED by every worker (the devices may still be running them). Everything but
// phd_step_async starts with this, and then drives the shards from the caller's thread as a single-device handle would.
static void multi_drain(MultiState* m)
{
	const long long target = m->posted.load(std::memory_order_acquire);
	for (int s = 0; s < m->n; s++) {
		for (long spins = 0; m->issued[s].load(std::memory_order_acquire) < target; spins++) {
			if (spins < 4096) cpu_pause();
			else std::this_thread::sleep_for(std::chrono::microseconds(50));
		}
	}
}

// ... and none of them failed: a step that could not be issued on some shard leaves the shards out of step with each other
// (some rotated, some not); the handle then refuses everything until phd_reset / phd_upload_state_soa replace the state.
static int multi_enter(phd_navigator* nav)
{
	MultiState* m = nav->multi;
	multi_drain(m);
	if (m->failed.load()) {
		std::lock_guard<std::mutex> g(m->mu);
		return nav->fail(m->fail_code, "a step could not be issued on device " + std::to_string(m->sh[m->fail_shard]->device) + " (shard " + std::to_string(m->fail_shard) +
		                 "): " + m->fail_msg + " — the shards are out of step; phd_reset or phd_upload_state_soa starts over");
	}
	return PHD_OK;
}

static void multi_worker_fail(MultiState* m, int s, int rc)
{
	std::lock_guard<std::mutex> g(m->mu);
	if (!m->failed.load()) {
		m->fail_code = rc; m->fail_shard = s; m->fail_msg = m->sh[s]->err;
		m->failed.store(1);
	}
}

// One SlamUpdate of shard s (see the head of this file), issued by its worker.
static void multi_issue_step(MultiState* m, int s, long long k, const MultiCmd& c)
{
	phd_navigator* a = m->sh[s];
	const int n = m->n, par = (int) (k & 1);
	const auto t0 = std::chrono::steady_clock::now();
	hipEvent_t* pe = nullptr;
	if (s == 0 && m->ph_on && m->ph_made && m->ph_count < MULTI_PH_SAMPLES && (k % m->ph_period) == 0) pe = m->ph_ev[m->ph_count];
	int rc = PHD_OK;
	if (!m->failed.load()) {
		if (pe) hipEventRecord(pe[0], a->stream);
		rc = step_local(a, c.onlymapping);
		if (!rc && hipEventRecord(m->ev_gather[par][s], a->stream) != hipSuccess) rc = a->fail(PHD_ERR_DEVICE, "hipEventRecord (gather)");
		if (pe) hipEventRecord(pe[1], a->stream);
		if (rc) multi_worker_fail(m, s, rc);
	}
	m->gather_rec[s].store(k + 1, std::memory_order_release);
	double spun = 0;
	for (int t = 0; t < n; t++) {
		if (t == s) continue;
		if (m->gather_rec[t].load(std::memory_order_acquire) < k + 1) {   // the owner has recorded this step's event (or given up)
			const auto w0 = std::chrono::steady_clock::now();
			if (!multi_wait_counter(m->gather_rec[t], k + 1)) {
				a->fail(PHD_ERR_DEVICE, "shard " + std::to_string(t) + "'s worker did not record its weight event within a minute");
				multi_worker_fail(m, s, PHD_ERR_DEVICE);
			}
			spun += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count();
		}
		if (!m->failed.load() && hipStreamWaitEvent(a->stream, m->ev_gather[par][t], 0) != hipSuccess) {
			a->fail(PHD_ERR_DEVICE, "hipStreamWaitEvent (gather)");
			multi_worker_fail(m, s, PHD_ERR_DEVICE);
		}
	}
	if (!m->failed.load()) {
		if (pe) hipEventRecord(pe[2], a->stream);
		rc = step_global(a, s, n, c.u, c.onlymapping, false);
		if (pe) hipEventRecord(pe[3], a->stream);
		if (!rc) {
			// every record straight into its place in the receiver's buffer (how many there are is known on the device)
			StepBufs b = make_bufs(a);
			launch_timed(a, T_PK, a->stream, false, k_pack_particles, dim3(pack_grid(a)), dim3(256), 0, b, a->plan, n, (double*) nullptr, (double* const*) a->d_recv_tab);
			if (hipGetLastError() != hipSuccess) rc = a->fail(PHD_ERR_DEVICE, "k_pack_particles");
		}
		if (!rc && hipEventRecord(m->ev_pack[par][s], a->stream) != hipSuccess) rc = a->fail(PHD_ERR_DEVICE, "hipEventRecord (pack)");
		if (pe) hipEventRecord(pe[4], a->stream);
		if (rc) multi_worker_fail(m, s, rc);
	}
	m->pack_rec[s].store(k + 1, std::memory_order_release);
	for (int t = 0; t < n; t++) {
		if (t == s) continue;
		if (m->pack_rec[t].load(std::memory_order_acquire) < k + 1) {
			const auto w0 = std::chrono::steady_clock::now();
			if (!multi_wait_counter(m->pack_rec[t], k + 1)) {
				a->fail(PHD_ERR_DEVICE, "shard " + std::to_string(t) + "'s worker did not record its pack event within a minute");
				multi_worker_fail(m, s, PHD_ERR_DEVICE);
			}
			spun += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - w0).count();
		}
		if (!m->failed.load() && hipStreamWaitEvent(a->stream, m->ev_pack[par][t], 0) != hipSuccess) {
			a->fail(PHD_ERR_DEVICE, "hipStreamWaitEvent (pack)");
			multi_worker_fail(m, s, PHD_ERR_DEVICE);
		}
	}
	if (!m->failed.load()) {
		rc = step_finish(a);
		if (pe) { hipEventRecord(pe[5], a->stream); m->ph_count++; }
		if (rc) multi_worker_fail(m, s, rc);
	}
	m->issue_us[s] += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
	m->spin_us[s] += spun;
	if (s == 0) m->issue_steps++;
}

static void multi_worker(MultiState* m, int s)
{
	hipSetDevice(m->sh[s]->device);
	for (long long k = 0;; k++) {
		// the next step: a short spin (steps come back to back in a batch), then sleep until one is posted
		for (int spins = 0; m->posted.load(std::memory_order_acquire) <= k && !m->stop.load() && spins < 20000; spins++) cpu_pause();
		if (m->posted.load(std::memory_order_acquire) <= k && !m->stop.load()) {
			std::unique_lock<std::mutex> g(m->mu);
			m->cv_work.wait(g, [&] { return m->posted.load(std::memory_order_acquire) > k || m->stop.load(); });
		}
		if (m->posted.load(std::memory_order_acquire) <= k) return;   // stop, and nothing left to issue
		const MultiCmd c = m->ring[k % MULTI_RING];
		multi_issue_step(m, s, k, c);
		m->issued[s].store(k + 1, std::memory_order_release);
	}
}

void multi_destroy(phd_navigator* nav)
{
	MultiState* m = nav->multi;
	if (!m->workers.empty()) {
		multi_drain(m);
		{
			std::lock_guard<std::mutex> g(m->mu);
			m->stop.store(1);
		}
		m->cv_work.notify_all();
		for (std::thread& t : m->workers) t.join();
	}
	for (size_t s = 0; s < m->sh.size(); s++) {
		if (!m->sh[s]) continue;
		hipSetDevice(m->sh[s]->device);
		hipStreamSynchronize(m->sh[s]->stream);
		for (int q = 0; q < 2; q++) {
			if (s < m->ev_gather[q].size() && m->ev_gather[q][s]) hipEventDestroy(m->ev_gather[q][s]);
			if (s < m->ev_pack[q].size() && m->ev_pack[q][s]) hipEventDestroy(m->ev_pack[q][s]);
		}
	}
	if (m->ph_made) {
		hipSetDevice(m->sh[0]->device);
		for (int i = 0; i < MULTI_PH_SAMPLES; i++) for (int q = 0; q < 6; q++) hipEventDestroy(m->ph_ev[i][q]);
	}
	for (size_t s = 0; s < m->sh.size(); s++) if (m->sh[s]) phd_destroy(m->sh[s]);
	delete m;
	delete nav;
}

extern "C" phd_navigator* phd_create_multi(const phd_params* params, const int* devices, int ndevices)
{
	g_create_error.clear();
	if (!params || !devices || ndevices < 1 || ndevices > PHD_MAX_DEVICES) { g_create_error = "phd_create_multi: params / devices NULL or device count out of 1..64"; return nullptr; }
	if (params->max_particles < ndevices || params->max_particles % ndevices) {
		g_create_error = "phd_create_multi: max_particles must be a multiple of the device count (equal shards)";
		return nullptr;
	}
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_error = "no HIP device: libphdhip has no CPU path"; return nullptr; }
	for (int s = 0; s < ndevices; s++) {
		if (devices[s] < 0 || devices[s] >= ndev) { g_create_error = "phd_create_multi: bad device ordinal " + std::to_string(devices[s]); return nullptr; }
	}
	// The shards store into each other's memory from kernels: every pair of distinct devices needs direct peer access
	// (xGMI or PCIe P2P). Without it there is no slower path to fall back to silently: the call fails and says which pair.
	// (enabled before anything is allocated, so that every allocation of a shard is mapped for its peers)
	std::vector<uint8_t> p2p((size_t) ndevices * ndevices, 0);
	for (int s = 0; s < ndevices; s++) {
		if (hipSetDevice(devices[s]) != hipSuccess) { g_create_error = "phd_create_multi: hipSetDevice(" + std::to_string(devices[s]) + ") failed"; return nullptr; }
		for (int t = 0; t < ndevices; t++) {
			if (devices[t] == devices[s]) { p2p[(size_t) s * ndevices + t] = 1; continue; }
			int can = 0;
			if (hipDeviceCanAccessPeer(&can, devices[s], devices[t]) != hipSuccess || !can) {
				(void) hipGetLastError();
				g_create_error = "phd_create_multi: device " + std::to_string(devices[s]) + " has no direct peer access to device " + std::to_string(devices[t]) +
				                 " (hipDeviceCanAccessPeer): the shards exchange weights and particles by peer stores and there is no staged path — "
				                 "use devices that reach each other over xGMI / PCIe P2P, or one process per GPU with RCCL";
				return nullptr;
			}
			const hipError_t e = hipDeviceEnablePeerAccess(devices[t], 0);
			if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
				g_create_error = "phd_create_multi: hipDeviceEnablePeerAccess(" + std::to_string(devices[s]) + " -> " + std::to_string(devices[t]) + "): " + hipGetErrorString(e);
				(void) hipGetLastError();
				return nullptr;
			}
			(void) hipGetLastError();
			p2p[(size_t) s * ndevices + t] = 1;
		}
	}
	phd_navigator* nav = new phd_navigator();
	nav->multi = new MultiState();
	nav->prm = *params;
	nav->device = devices[0];
	nav->Pcap = params->max_particles;
	MultiState* m = nav->multi;
	m->n = ndevices;
	m->devices.assign(devices, devices + ndevices);
	m->p2p = p2p;
	m->shard_cap = params->max_particles / ndevices;
	phd_params sp = *params;
	sp.max_particles = m->shard_cap;
	for (int q = 0; q < 2; q++) { m->ev_gather[q].assign(ndevices, nullptr); m->ev_pack[q].assign(ndevices, nullptr); }
	for (int s = 0; s < ndevices; s++) {
		phd_navigator* sh = phd_create(&sp, devices[s]);
		if (!sh) {
			g_create_error = "phd_create_multi: device " + std::to_string(devices[s]) + ": " + g_create_error;
			multi_destroy(nav);
			return nullptr;
		}
		m->sh.push_back(sh);
		hipSetDevice(devices[s]);
		bool ok = true;
		for (int q = 0; q < 2; q++) {
			ok = ok && hipEventCreateWithFlags(&m->ev_gather[q][s], hipEventDisableTiming) == hipSuccess;
			ok = ok && hipEventCreateWithFlags(&m->ev_pack[q][s], hipEventDisableTiming) == hipSuccess;
		}
		// the buffers other shards will know by address: gathered weights (+ status words), receive buffer
		ok = ok && ensure_sharded(sh, false) == PHD_OK && ensure_gw(sh, params->max_particles, true) == PHD_OK;
		ok = ok && hipMemset(sh->d_gw, 0, ((size_t) params->max_particles + PHD_MAX_DEVICES) * 8) == hipSuccess;
		if (!ok) {
			g_create_error = "phd_create_multi: device " + std::to_string(devices[s]) + ": " + (sh->err.empty() ? std::string(hipGetErrorString(hipGetLastError())) : sh->err);
			multi_destroy(nav);
			return nullptr;
		}
	}
	// every shard's tables: where its weights go (all gathered vectors) and where its migrating particles go (all receive buffers)
	std::vector<double*> gwt(ndevices), rvt(ndevices);
	for (int t = 0; t < ndevices; t++) { gwt[t] = m->sh[t]->d_gw; rvt[t] = m->sh[t]->d_recv; }
	for (int s = 0; s < ndevices; s++) {
		phd_navigator* sh = m->sh[s];
		hipSetDevice(devices[s]);
		bool ok = hipMemcpy(sh->d_recv_tab, rvt.data(), ndevices * sizeof(double*), hipMemcpyHostToDevice) == hipSuccess;   // (the table itself: ensure_sharded)
		ok = ok && hipMemcpy(sh->d_dst_tab, gwt.data(), ndevices * sizeof(double*), hipMemcpyHostToDevice) == hipSuccess;
		if (!ok) { g_create_error = "phd_create_multi: table upload failed"; multi_destroy(nav); return nullptr; }
		sh->ndst = ndevices;
		sh->peers_set = true;
		sh->gw_shared = true;
		sh->push_flagslot = params->max_particles + s;
		sh->d_gflags = sh->d_gw + params->max_particles;
	}
	hipSetDevice(devices[0]);
	bool okp = true;
	for (int i = 0; i < MULTI_PH_SAMPLES && okp; i++) for (int q = 0; q < 6 && okp; q++) okp = hipEventCreate(&m->ph_ev[i][q]) == hipSuccess;
	m->ph_made = okp;
	m->issued.reset(new std::atomic<long long>[ndevices]);
	m->gather_rec.reset(new std::atomic<long long>[ndevices]);
	m->pack_rec.reset(new std::atomic<long long>[ndevices]);
	m->issue_us.reset(new double[ndevices]);
	m->spin_us.reset(new double[ndevices]);
	for (int s = 0; s < ndevices; s++) { m->issued[s].store(0); m->gather_rec[s].store(0); m->pack_rec[s].store(0); m->issue_us[s] = 0; m->spin_us[s] = 0; }
	for (int s = 0; s < ndevices; s++) m->workers.emplace_back(multi_worker, m, s);
	return nav;
}

static int multi_particles_ok(phd_navigator* nav, int nparticles, const char* who)
{
	const int n = nav->multi->n;
	if (nparticles < n || nparticles > nav->Pcap || nparticles % n) {
		return nav->fail(PHD_ERR_BAD_ARGUMENT, std::string(who) + ": the particle count must be a multiple of the device count (" + std::to_string(n) + ") within max_particles");
	}
	return PHD_OK;
}

// a new particle set: shard s's weights go to offset s * Pl of the gathered vectors; whatever kept the handle from stepping is gone
static void multi_new_state(phd_navigator* nav, int nparticles)
{
	MultiState* m = nav->multi;
	m->Pl = nparticles / m->n;
	for (int s = 0; s < m->n; s++) m->sh[s]->push_first = s * m->Pl;
	nav->P = nparticles;
	std::lock_guard<std::mutex> g(m->mu);
	m->failed.store(0);
	m->fail_code = PHD_OK;
}

int multi_reset(phd_navigator* nav, int nparticles, const double* pose7, const double* w, const double* mean3, const double* cov9, int ncomp)
{
	MultiState* m = nav->multi;
	multi_drain(m);
	int rc = multi_particles_ok(nav, nparticles, "phd_reset");
	if (rc) return rc;
	for (int s = 0; s < m->n; s++) {
		rc = reset_impl(m->sh[s], nparticles / m->n, pose7, w, mean3, cov9, ncomp, 1.0 / nparticles);
		if (rc) return multi_fail_from(nav, m->sh[s], rc, s);
	}
	multi_new_state(nav, nparticles);
	return PHD_OK;
}

int multi_set_small(phd_navigator* nav, const double* poses7, const double* weights, int nparticles)
{
	MultiState* m = nav->multi;
	int rc = multi_enter(nav);
	if (rc) return rc;
	if (nparticles != nav->P || (!poses7 && !weights)) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_set_poses / phd_set_weights: particle count mismatch");
	for (size_t s = 0; s < m->sh.size(); s++) {
		rc = poses7 ? phd_set_poses(m->sh[s], poses7 + s * m->Pl * 7, m->Pl) : phd_set_weights(m->sh[s], weights + s * m->Pl, m->Pl);
		if (rc) return multi_fail_from(nav, m->sh[s], rc, (int) s);
	}
	return PHD_OK;
}

int multi_update_motion(phd_navigator* nav, const double* odometry6, const double* noise6, int nparticles, uint8_t perfect_still)
{
	MultiState* m = nav->multi;
	int rc = multi_enter(nav);
	if (rc) return rc;
	if (nparticles != nav->P) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_update_motion: particle count mismatch");
	for (size_t s = 0; s < m->sh.size(); s++) {
		rc = phd_update_motion(m->sh[s], odometry6, noise6 ? noise6 + s * m->Pl * 6 : nullptr, m->Pl, perfect_still);
		if (rc) return multi_fail_from(nav, m->sh[s], rc, (int) s);
	}
	return PHD_OK;
}

int multi_set_map(phd_navigator* nav, int particle, const double* w, const double* mean3, const double* cov9, int ncomp)
{
	MultiState* m = nav->multi;
	int rc = multi_enter(nav);
	if (rc) return rc;
	if (particle < 0 || particle >= nav->P) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_set_map: particle out of range");
	const int s = particle / m->Pl;
	rc = phd_set_map(m->sh[s], particle - s * m->Pl, w, mean3, cov9, ncomp);
	return rc ? multi_fail_from(nav, m->sh[s], rc, s) : PHD_OK;
}

int multi_upload(phd_navigator* nav, int nparticles, int stride, const double* planes, const int32_t* counts, const double* poses7, const double* weights)
{
	MultiState* m = nav->multi;
	multi_drain(m);
	int rc = multi_particles_ok(nav, nparticles, "phd_upload_state_soa");
	if (rc) return rc;
	const int n = m->n, Pl = nparticles / n;
	for (int s = 0; s < n; s++) {
		const size_t first = (size_t) s * Pl;
		rc = upload_impl(m->sh[s], Pl, stride, planes + first * stride, (size_t) nparticles * stride, counts + first, poses7 + first * 7, weights + first);
		if (rc) return multi_fail_from(nav, m->sh[s], rc, s);
	}
	multi_new_state(nav, nparticles);
	return PHD_OK;
}

int multi_download(phd_navigator* nav, int stride, double* planes, int32_t* counts, double* poses7, double* weights)
{
	MultiState* m = nav->multi;
	int rc = multi_enter(nav);
	if (rc) return rc;
	for (size_t s = 0; s < m->sh.size(); s++) {
		const size_t first = s * m->Pl;
		rc = download_impl(m->sh[s], stride, planes + first * stride, (size_t) nav->P * stride, counts + first,
		                   poses7 ? poses7 + first * 7 : nullptr, weights ? weights + first : nullptr);
		if (rc) return multi_fail_from(nav, m->sh[s], rc, (int) s);
	}
	return PHD_OK;
}

int multi_set_measurements(phd_navigator* nav, const double* z3, int nmeasurements)
{
	MultiState* m = nav->multi;
	int rc = multi_enter(nav);
	if (rc) return rc;
	for (size_t s = 0; s < m->sh.size(); s++) {
		rc = phd_set_measurements(m->sh[s], z3, nmeasurements);
		if (rc) return multi_fail_from(nav, m->sh[s], rc, (int) s);
	}
	m->M = nmeasurements;
	return PHD_OK;
}

// every shard gets the whole map (each evaluates its own particles' components against it)
int multi_set_depth_map(phd_navigator* nav, const float* depth, int width, int height)
{
	MultiState* m = nav->multi;
	int rc = multi_enter(nav);
	if (rc) return rc;
	for (size_t s = 0; s < m->sh.size(); s++) {
		rc = phd_set_depth_map(m->sh[s], depth, width, height);
		if (rc) return multi_fail_from(nav, m->sh[s], rc, (int) s);
	}
	return PHD_OK;
}

int multi_forward_int(phd_navigator* nav, int what, long long value)
{
	MultiState* m = nav->multi;
	int rc = multi_enter(nav);
	if (rc) return rc;
	for (size_t s = 0; s < m->sh.size(); s++) {
		rc = what == 0 ? phd_set_split(m->sh[s], (int) value) : (what == 1 ? phd_set_association_workspace(m->sh[s], value) :
		     (what == 2 ? phd_set_frozen(m->sh[s], (uint8_t) value) : phd_set_all_pairs(m->sh[s], (uint8_t) value)));
		if (rc) return multi_fail_from(nav, m->sh[s], rc, (int) s);
	}
	return PHD_OK;
}

// phd_step_async on a multi-device handle: the step is posted to the workers and the call returns (it waits only when
// MULTI_RING steps are posted and not yet issued). What a step finds — a raised flag, a failed launch — surfaces at phd_sync.
int multi_step(phd_navigator* nav, uint8_t onlymapping, double u)
{
	MultiState* m = nav->multi;
	const auto t0 = std::chrono::steady_clock::now();
	if (nav->P < 1) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_step: no particles (call phd_reset first)");
	if (m->failed.load()) return multi_enter(nav);
	const long long k = m->posted.load(std::memory_order_relaxed);
	for (int s = 0; s < m->n; s++) {
		for (long spins = 0; k - m->issued[s].load(std::memory_order_acquire) >= MULTI_RING; spins++) {
			if (spins < 4096) cpu_pause();
			else std::this_thread::sleep_for(std::chrono::microseconds(20));
		}
	}
	m->ring[k % MULTI_RING] = MultiCmd{onlymapping, u};
	{
		std::lock_guard<std::mutex> g(m->mu);
		m->posted.store(k + 1, std::memory_order_release);
	}
	m->cv_work.notify_all();
	m->post_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
	m->posts++;
	return PHD_OK;
}

int multi_sync(phd_navigator* nav)
{
	MultiState* m = nav->multi;
	int rc = multi_enter(nav);
	if (rc) return rc;
	int first = PHD_OK, fs = 0;
	for (int s = 0; s < m->n; s++) {
		phd_navigator* a = m->sh[s];
		rc = phd_sync(a);
		if (!rc && a->plan.counts && a->sharded_used) {   // what the device plan of the last step said
			int st = MIG_OK;
			hipSetDevice(a->device);
			if (hipMemcpy(&st, a->plan.counts + mig_word(m->n, MC_STATUS), 4, hipMemcpyDeviceToHost) != hipSuccess) rc = a->fail(PHD_ERR_DEVICE, "reading the migration plan's status failed");
			else if (st == MIG_BAD) rc = a->fail(PHD_ERR_GENERIC, "the gathered source vector was not a resampling result");
			else if (st == MIG_OVERFLOW) rc = a->fail(PHD_ERR_CAPACITY, "more migrating particles than the send list holds");
		}
		if (rc && !first) { first = rc; fs = s; }
	}
	return first ? multi_fail_from(nav, m->sh[fs], first, fs) : PHD_OK;
}

const double* multi_weights(phd_navigator* nav, int* length)
{
	MultiState* m = nav->multi;
	if (multi_enter(nav)) return nullptr;
	m->h_weights.resize(std::max(nav->P, 1));
	for (size_t s = 0; s < m->sh.size(); s++) {
		int len = 0;
		const double* w = phd_weights(m->sh[s], &len);
		if (!w || len != m->Pl) return nullptr;
		std::memcpy(m->h_weights.data() + s * m->Pl, w, (size_t) len * 8);
	}
	if (length) *length = nav->P;
	return m->h_weights.data();
}

const double* multi_poses(phd_navigator* nav, int* length)
{
	MultiState* m = nav->multi;
	if (multi_enter(nav)) return nullptr;
	m->h_poses.resize((size_t) std::max(nav->P, 1) * 7);
	for (size_t s = 0; s < m->sh.size(); s++) {
		int len = 0;
		const double* q = phd_poses(m->sh[s], &len);
		if (!q || len != m->Pl * 7) return nullptr;
		std::memcpy(m->h_poses.data() + s * m->Pl * 7, q, (size_t) len * 8);
	}
	if (length) *length = nav->P * 7;
	return m->h_poses.data();
}

int multi_best_particle(phd_navigator* nav)
{
	if (multi_sync(nav)) return -1;
	return phd_best_particle(nav->multi->sh[0]);   // a slot of the whole particle set (every shard computed the same one)
}

int multi_map(phd_navigator* nav, int particle, int* ncomp, const double** w, const double** mean3, const double** cov9)
{
	MultiState* m = nav->multi;
	int rc = multi_enter(nav);
	if (rc) return rc;
	if (particle < 0 || particle >= nav->P || !ncomp) return nav->fail(PHD_ERR_BAD_ARGUMENT, "phd_map: particle out of range");
	const int s = particle / m->Pl;
	rc = phd_map(m->sh[s], particle - s * m->Pl, ncomp, w, mean3, cov9);
	return rc ? multi_fail_from(nav, m->sh[s], rc, s) : PHD_OK;
}

// global source slot of every particle in the last step (identity when no resampling happened): every shard holds the
// whole vector, shard 0's is read
const int32_t* multi_resample_sources(phd_navigator* nav, int* length, uint8_t* resampled)
{
	MultiState* m = nav->multi;
	if (multi_sync(nav)) return nullptr;
	phd_navigator* a = m->sh[0];
	m->h_src.resize(std::max(nav->P, 1));
	hipSetDevice(a->device);
	int info[2] = {0, 0};
	if (hipMemcpy(info, a->d_info, 8, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
	if (info[1] && a->sharded_used && a->last_world_particles == nav->P) {
		if (hipMemcpy(m->h_src.data(), a->d_plan, (size_t) nav->P * 4, hipMemcpyDeviceToHost) != hipSuccess) return nullptr;
	}
	else {
		for (int i = 0; i < nav->P; i++) m->h_src[i] = i;
	}
	if (length) *length = nav->P;
	if (resampled) *resampled = info[1] ? 1 : 0;
	return m->h_src.data();
}

phd_navigator* multi_shard0(phd_navigator* nav)
{
	multi_drain(nav->multi);
	return nav->multi->sh[0];
}

// Diagnostics of the multi-device host (bench.py --single-process), nine doubles: out[0..4] mean device time, in ms, of the phases of the
// sampled steps on shard 0's stream — local step (its kernels + the weight stores) | waiting for the other shards' weights |
// global resampling + plan | pack (peer stores of the migrating particles) | waiting for the other shards' records + unpack;
// out[5] mean time the caller's thread spent inside phd_step_async (us); out[6] mean time a worker spent issuing one step
// (us; the slowest shard); out[7] sampled steps; out[8] the same as [6] without the time spent waiting for the other workers
// to record their events (the HIP calls alone). Sampling follows phd_timing_reset (every n-th step). p2p (may be NULL):
// [n][n] bytes, 1 where shard s reaches shard t's memory directly.
extern "C" int phd_multi_report(phd_navigator* nav, double* out8, uint8_t* p2p, int* nshards)
{
	if (!nav || !nav->multi || !out8) return PHD_ERR_BAD_ARGUMENT;
	MultiState* m = nav->multi;
	multi_drain(m);
	for (int q = 0; q < 9; q++) out8[q] = 0;
	hipSetDevice(m->sh[0]->device);
	hipStreamSynchronize(m->sh[0]->stream);
	int got = 0;
	for (int i = 0; i < m->ph_count; i++) {
		float f[5];
		bool ok = true;
		for (int q = 0; q < 5 && ok; q++) ok = hipEventElapsedTime(&f[q], m->ph_ev[i][q], m->ph_ev[i][q + 1]) == hipSuccess;
		if (!ok) { (void) hipGetLastError(); continue; }
		for (int q = 0; q < 5; q++) out8[q] += f[q];
		got++;
	}
	for (int q = 0; q < 5; q++) out8[q] /= std::max(got, 1);
	out8[5] = m->posts ? m->post_us / (double) m->posts : 0;
	double worst = 0, worst_api = 0;
	for (int s = 0; s < m->n; s++) { worst = std::max(worst, m->issue_us[s]); worst_api = std::max(worst_api, m->issue_us[s] - m->spin_us[s]); }
	out8[6] = m->issue_steps ? worst / (double) m->issue_steps : 0;
	out8[7] = got;
	out8[8] = m->issue_steps ? worst_api / (double) m->issue_steps : 0;
	if (p2p) std::memcpy(p2p, m->p2p.data(), m->p2p.size());
	if (nshards) *nshards = m->n;
	return PHD_OK;
}

// (phd_timing_reset on a multi-device handle also restarts these)
static void multi_timing_reset(phd_navigator* nav, uint8_t enabled)
{
	MultiState* m = nav->multi;
	multi_drain(m);
	m->ph_on = enabled != 0;
	m->ph_period = enabled ? enabled : 1;
	m->ph_count = 0;
	m->post_us = 0; m->posts = 0; m->issue_steps = 0;
	for (int s = 0; s < m->n; s++) { m->issue_us[s] = 0; m->spin_us[s] = 0; }
}
