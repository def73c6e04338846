/*
 * phdhip.h — C-ABI of libphdhip.so, the MI355X (gfx950) implementation of monorfs's
 * Rao-Blackwellized PHD-SLAM inner loop.
 *
 * The library sits behind the reference's solver interface
 *     abstract class Navigator<MeasurerT, PoseT, MeasurementT>
 *     (mono-rfs-lib/SLAM/Navigators/Navigator.cs:47-396)
 * and replaces the managed body of
 *     PHDNavigator.SlamUpdate (mono-rfs-lib/SLAM/Navigators/PHDNavigator.cs:323-362)
 * for the PRM3D model (Pose3D + PixelRangeMeasurement). The calling convention mirrors the
 * reference's only native solver binding, ISAM2Lib (ISAM2Navigator.cs:600-622 <-> isam2/isam2.cpp:46-365):
 *   - an opaque handle made by a `create` call and released by a `destroy` call;
 *   - inputs are caller-owned flat `double*` / `int*`, read only for the duration of the call;
 *   - outputs are library-owned host buffers returned as pointer + length, valid until the next
 *     call on the same handle (the C# side copies them out, ISAM2Navigator.cs:507-593);
 *   - booleans cross as one byte (UnmanagedType.U1, ISAM2Navigator.cs:609);
 *   - every call returns an int status: 0 ok, >0 a specific condition, -1 generic failure
 *     (isam2.cpp:317-335); no C++ exception ever crosses the boundary.
 *
 * Threading: one caller thread per handle, no re-entrancy (Simulation.Update drives the
 * navigator from one thread, Simulation.cs:636-673). The library uses HIP streams internally.
 *
 * Non-finite input: measurements, poses, weights, odometry, noise and map components that are NaN or infinite are rejected
 * with PHD_ERR_BAD_ARGUMENT by every call that takes them (the state is untouched). The reference would carry a NaN through
 * its weight sums (PHDNavigator.cs:886-890) and end with NaN particle weights; the device's pair loops count a NaN exponent
 * as exp(-800) = 0. With finite input the two agree, so the boundary keeps the other case out.
 *
 * Matrix conventions: row-major; a 3-D Gaussian component is (weight, mean[3], cov[9]);
 * a pose is (x, y, z, qw, qx, qy, qz) as in Pose3D (Pose3D.cs:142-162); a measurement is
 * (px, py, range) as in PixelRangeMeasurement.ToLinear (PixelRangeMeasurement.cs:96-99).
 */
#ifndef PHDHIP_H
#define PHDHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHD_API_VERSION 4   /* 2: phd_create_multi, phd_set_association_workspace; phd_migration_local_async gone
                               3: phd_multi_report; phd_device_local_weights is an export buffer; the migration plan is made on the device
                               4: the sharded step without a host wait (phd_step_global_device_async, phd_migration_push_async, the IPC
                                  calls); phd_device_local_weights holds P + 1 doubles; the device keeps one 80-byte record per component
                               (4, added: phd_set_depth_map / phd_test_detection_probability, the Kinect model; hosts detect them by symbol) */

/* status codes */
#define PHD_OK                    0
#define PHD_ERR_GENERIC          -1
#define PHD_ERR_BAD_ARGUMENT      1   /* a size/pointer/flag is out of range                        */
#define PHD_ERR_CAPACITY          2   /* a mixture outgrew its slab (raise max_components/emit_cap); the step is dropped,
                                         the state is the one before it                              */
#define PHD_ERR_ASSOCIATION       3   /* a data-association cluster of more than 256 rows, or the clusters beyond 64 rows
                                         used up the association workspace; surfaces as Data["module"]="association"
                                         (Simulation.cs:666). The step is dropped, the state is the one before it.   */
#define PHD_ERR_DEVICE            4   /* HIP runtime error, see phd_last_error                       */
#define PHD_ERR_NO_DEVICE         5   /* no gfx950 device / HIP runtime unavailable                  */

/* dynamics model. PRM3D is the product. LINEAR2D is the toy model of the reference's unit tests (PHDNavigatorTest.cs):
 * it runs through the same kernels — a pose is (x, y, 0, 1, 0, 0, 0), a measurement (x, y, 0), still three doubles, R is
 * 2 x 2 row-major in the first four entries of `R` — so that those tests' vectors can be put to the device itself.
 * phd_update_motion is PRM3D only; the gradient of phd_quasi_set_loglik_grad has its first two entries for (x, y).  */
#define PHD_MODEL_LINEAR2D 0
#define PHD_MODEL_PRM3D    1

/* radius-gate metric of Map.Near / Map.Evaluate(x, r) (Map.cs:170-184, 210-220): the reference
 * delegates to Accord 3.0.2 KDTree.Nearest(point, radius), whose metric is not in the tree.   */
#define PHD_GATE_SQUARED_EUCLIDEAN 1  /* |x-m|^2 <= radius   (Accord 3.0.x default distance) */
#define PHD_GATE_EUCLIDEAN         0  /* |x-m|   <= radius                                   */
#define PHD_GATE_DISABLED          2  /* every component is "near" (PHDNavigatorTest.Correct) */

/*
 * Every configuration value the path reads. Field <- reference origin:
 */
typedef struct phd_params {
	int32_t model;                 /* Config.Model (Config.cs:47)                                      */
	int32_t zdim;                  /* measurement dimension: 3 for PRM3D, 2 for Linear2D               */
	double  measurer[7];           /* PRM3DMeasurer.ToLinear(): focal, rangemin, rangemax, filmX, filmY,
	                                  filmW, filmH (PRM3DMeasurer.cs:92-96); rangemin/max are float32
	                                  values widened to double (PRM3DMeasurer.cs:65,73).
	                                  Linear2D: measurer[0] = Range (Linear2DMeasurer.cs:56-59)        */
	double  R[9];                  /* MeasurementCovariance * MeasurementCovarianceMultiplier, zdim x zdim
	                                  row-major in the leading entries (SimulatedVehicle.cs:159-168)  */
	double  visibility_ramp[3];    /* Config.VisibilityRamp (Config.cs:257-259)                        */
	double  pd;                    /* Config.NavigatorPD (Config.cs:90)                                */
	double  clutter_density;       /* Config.NavigatorClutterDensity (Config.cs:91)                    */
	double  birth_covariance[9];   /* Config.BirthCovariance (Config.cs:77-79)                         */
	double  birth_weight;          /* Config.BirthWeight (Config.cs:80)                                */
	double  min_weight;            /* Config.MinWeight (Config.cs:81)                                  */
	double  min_effective_particle;/* Config.MinEffectiveParticle (Config.cs:82)                       */
	int32_t max_quantity;          /* Config.MaxQuantity (Config.cs:83)                                */
	int32_t gate_metric;           /* PHD_GATE_*                                                       */
	double  merge_threshold;       /* Config.MergeThreshold (Config.cs:84)                             */
	double  exploration_threshold; /* Config.ExplorationThreshold (Config.cs:85)                       */
	double  density_distance_threshold; /* Config.DensityDistanceThreshold (Config.cs:74)              */
	/* capacities of the device slabs (not reference values) */
	int32_t max_particles;         /* particles this handle (this GPU's shard) can hold                */
	int32_t max_components;        /* components per particle slab, >= max_quantity                    */
	int32_t max_measurements;      /* measurements per frame                                           */
	int32_t emit_capacity;         /* per-particle scratch for corrected-but-unpruned components;
	                                  0 = library default                                              */
} phd_params;

typedef struct phd_navigator phd_navigator;

/* Fill `p` with the PRM3D defaults of Config.SetPRM3DDefaults (Config.cs:238-263) and the PHD
 * constants of Config.cs:74-91; capacities are set from the three arguments.                   */
void phd_default_params(phd_params* p, int max_particles, int max_components, int max_measurements);

/* ≙ `new PHDNavigator(vehicle, particlecount, onlymapping)` (PHDNavigator.cs:192-208) and
 * ISAM2Lib.newnavigator (ISAM2Navigator.cs:603). `device` is the HIP ordinal. NULL on failure;
 * phd_create_error() then holds the reason. max_quantity: up to the LDS bound, about 3400 (one
 * particle's prune keeps its working set in a workgroup's LDS; every row up to there is pruned).  */
phd_navigator* phd_create(const phd_params* params, int device);
/* The same over several devices of one node (SURVEY §8b "device list", §8e): ONE handle, ONE caller thread — what a C# host
 * can drive (Simulation.Update runs the solver from one thread, Simulation.cs:636-673; it has no RCCL). The particles are
 * sharded contiguously, ndevices equal shards: params->max_particles and every particle count are TOTALS and multiples of
 * ndevices. Inside, one worker thread per shard issues that shard's launches; the shards' kernels run concurrently, the
 * un-normalised weights (16 KB per pair at 2048 particles per GPU) and the migrating particles are stored by the kernels
 * straight into the other shards' memory over xGMI (peer stores into fine-grained buffers: no copy engine, no host call per
 * pair), the normalisation / BestParticle / systematic resampling and the migration plan are computed identically on every
 * device: results are bit-identical to a single-device handle holding all particles, for any ndevices. Every pair of
 * distinct devices must have direct peer access (the call fails, naming the pair, otherwise). A device may be listed more
 * than once (tests; the distinct-device path has not been run on hardware by the builder: one-GPU boxes).
 * Available on such a handle: phd_reset, phd_set_poses / _weights / _map, phd_update_motion, phd_slam_update,
 * phd_set_measurements / phd_step_async / phd_sync — phd_step_async only POSTS the step to the workers and returns (a ring
 * of 256 posted steps; nothing of a step waits for the host, what it finds surfaces at phd_sync) —, the getters, phd_upload /
 * download_state_soa, phd_set_frozen / _split / _all_pairs / _association_workspace, phd_quasi_set_loglik[_grad], phd_quasi_ascent, phd_resample /
 * phd_particle_depleted, the timing calls (first shard); the stage-level KAT entry points and the per-rank sharding primitives
 * below return PHD_ERR_BAD_ARGUMENT.                                                                                     */
phd_navigator* phd_create_multi(const phd_params* params, const int* devices, int ndevices);
/* Diagnostics of a multi-device handle (bench.py --single-process). out8 (NINE doubles): [0..4] mean device time (ms) of the phases of the
 * sampled steps on the first shard's stream — local step | waiting for the other shards' weights | global resampling + plan
 * | pack (peer stores of the migrating particles) | waiting for the other shards' records + unpack; [5] mean time the caller
 * spent inside phd_step_async (us); [6] mean time the slowest shard's worker spent issuing one step (us); [7] sampled steps
 * (phd_timing_reset(nav, n) samples every n-th step); [8] as [6] without the waits for the other workers' event records. p2p (may be NULL): [nshards][nshards] bytes, 1 where shard s stores
 * into shard t's memory directly (peer access or the same device; phd_create_multi fails when a pair cannot).        */
int            phd_multi_report(phd_navigator* nav, double* out8, uint8_t* p2p, int* nshards);
const char*    phd_create_error(void);
/* ≙ Navigator.Dispose (Navigator.cs:395) / ISAM2Lib.deletenavigator.                             */
void           phd_destroy(phd_navigator* nav);
const char*    phd_last_error(const phd_navigator* nav);
int            phd_api_version(void);

/* ≙ PHDNavigator.reset (PHDNavigator.cs:245-266): `nparticles` equal particles at `pose`, each
 * with a deep copy of the `ncomp`-component map and weight 1/nparticles; BestParticle = 0.
 * Also serves CollapseParticles (:233-236) and ResetMapModel (:271-276, ncomp = 0).              */
int phd_reset(phd_navigator* nav, int nparticles, const double* pose7,
              const double* w, const double* mean3, const double* cov9, int ncomp);

/* The host keeps the motion model and its RNG (TrackVehicle.UpdateNoisy, TrackVehicle.cs:89-102):
 * after Navigator.Update (PHDNavigator.cs:295-314) it hands the particle poses over.
 * Like phd_set_weights, phd_update_motion and phd_set_measurements this does NOT wait for the device: the caller's array is
 * copied into pinned staging (free again when the call returns), the copy to the device and the store into the current
 * state are enqueued on the handle's stream — correct right behind phd_step_async, because the bank holding the current
 * state is looked up on the device.                                                              */
int phd_set_poses(phd_navigator* nav, const double* poses7, int nparticles);
/* SURVEY row f1 (next to the path): the particle motion step itself on the device. TrackVehicle.UpdateNoisy
 * (TrackVehicle.cs:89-102) = Pose3D.AddOdometry (Pose3D.cs:314-333) of the reading (dx dy dz dpitch dyaw droll),
 * then of the particle's own noise vector noise6[i*6..] = dt * chol(MotionCovariance) * N(0, I) drawn by the host
 * (Util.cs:173-202; NULL: none). perfect_still: a zero reading skips the noise (SimulatedVehicle.cs:190-202).
 * Replaces the per-frame phd_set_poses upload.                                                   */
int phd_update_motion(phd_navigator* nav, const double* odometry6, const double* noise6, int nparticles,
                      uint8_t perfect_still);
/* Test/bench access to the public arrays VehicleWeights / MapModels (PHDNavigator.cs:128,134). A resampling step
 * leaves the copies of a particle sharing their source's map (the deep copies of :740-741 are an index on the device):
 * phd_set_map therefore first gathers every map into its own place, one pass over the state (phd_map does not).   */
int phd_set_weights(phd_navigator* nav, const double* weights, int nparticles);
int phd_set_map(phd_navigator* nav, int particle, const double* w, const double* mean3,
                const double* cov9, int ncomp);

/* ≙ PHDNavigator.SlamUpdate (PHDNavigator.cs:323-362): predict, correct, prune and (unless
 * `onlymapping`) reweight every particle, then normalise, pick BestParticle and resample if
 * depleted. `u_resample` replaces `(double) Util.Uniform.Next()` of ResampleParticles
 * (PHDNavigator.cs:727): the RNG stays on the host. Blocking.                                    */
int phd_slam_update(phd_navigator* nav, const double* z3, int nmeasurements,
                    uint8_t onlymapping, double u_resample);

/* The same step split so that measurements can be resident before a timed region, or so that a 30 Hz host never
 * waits inside a frame: upload (asynchronous), enqueue (asynchronous on the handle's stream), wait + collect status.
 * Steps may be queued back to back; a failed one is dropped as a whole together with those queued behind it, and
 * phd_sync reports it. Up to 512 particles (environment PHD_CHAIN_MAX) the per-particle part of a step is one kernel
 * launch (up to 256 — PHD_DSPLIT_MAX, 0: never — with a second workgroup per particle that runs WeightAlpha's density sums beside
 * the association: the same results bit for bit). From 1024 particles on a step runs on two streams of the handle's own; phd_step_async directly behind
 * phd_step_async (no other call on the handle between them) is the fast path: the streams are not forked and joined around
 * each step, the end of a step runs on the stream that finishes last (results are bit-identical either way; any other call
 * on the handle, and a stream lent with phd_set_stream, take the fork / join order — INTEGRATION.md, "Posting steps back to
 * back").                                                                                         */
int phd_set_measurements(phd_navigator* nav, const double* z3, int nmeasurements);
/* Kinect input (KinectMeasurer.FuzzyVisibleM, KinectMeasurer.cs:151-173; PRM3D handles only, else PHD_ERR_BAD_ARGUMENT): the
 * current depth frame, row-major depth[y * width + x] with width = ResX and height = ResY (the reference's float[ResX][ResY]
 * depth[x][y], flattened), 1..PHD_DEPTH_MAX on each side. With a map, the detection probability of a pixel-range point
 * z = (X, Y, range) — everywhere the step evaluates it: the sweep, the Kalman emit and SetLogLikeMatrix; NOT the quasi set
 * log-likelihood (phd_quasi_set_loglik[_grad]), which keeps the constant pd as the reference does — is
 *     base = the PRM3D visibility clamped to [0, 1];  0 if base == 0
 *     x = (int) (X + (float) ResX / 2), y = (int) (Y + (float) ResY / 2)  (truncated; a pixel outside the image: 0)
 *     d = depth[y * width + x]; 0 if d is NaN ("no reading")
 *     r = (float) range;  m = min(base, (r - (float) rangemin) / ramp[2], (d - r) / ramp[2])  (float32 subtractions)
 *     PD = max(0, min(1, m)) * pd
 * Depth values are compared with the range as given, nothing is converted (units are the caller's); NaN and +-inf are
 * accepted here — the one exception to the non-finite rule above. The map is sticky: every step posted after the call uses
 * it until the next call; depth = NULL with 0 x 0 switches it off (exactly the PRM3D path again). The buffer is copied before
 * the call returns (pinned staging, an asynchronous copy on the handle's stream ordered before the next step); a map larger
 * than any before (re)allocates the device buffer, and that call waits for the handle's streams. A multi-device handle
 * gives every shard the whole map. A refused call (bad arguments) leaves the previous map in place, and so does a failed
 * allocation on a single-device handle.                                      */
#define PHD_DEPTH_MAX 4096
int phd_set_depth_map(phd_navigator* nav, const float* depth, int width, int height);
/* Test surface of the above: the device's detection probability (the step's own __device__ function, with the handle's
 * parameters and current map) at n pixel-range points z3[n][3] -> out[n]. Waits for the device.                        */
int phd_test_detection_probability(phd_navigator* nav, const double* z3, int n, double* out);
int phd_step_async(phd_navigator* nav, uint8_t onlymapping, double u_resample);
int phd_sync(phd_navigator* nav);
/* One mapping-only step that one particle sits out: in every respect phd_step_async(nav, 1, u) — the uniform is not used in
 * mapping mode — except that particle slot `held` has, behind the step, exactly the mixture it had in front of it, bit for
 * bit (component count, weights, means, covariances); its pose and weight are not touched. held == -1 holds nobody: the plain
 * mapping step. What it is for: the T leave-one-out filters of the smoother (LoopyPHDNavigator.FilterMissing,
 * LoopyPHDNavigator.cs:729-762, one per frame of UpdateMessagesFromMap :511-552) see the same poses and measurement sets and
 * differ in the one frame each skips, so they are T particles of one handle stepped together, particle k held at frame k
 * (LeaveOneOutMaps of the host mirrors; INTEGRATION.md, "Leave-one-out maps").
 * The hold is a copy of the slot's records out of the current state in front of the step and back behind it, by two small
 * kernels that look the current state up on the device (no step kernel knows of it): asynchronous, nothing waits for the
 * host, correct right behind phd_step_async (also one that resampled), phd_set_poses, phd_set_measurements and another
 * phd_step_hold_async. With 1024 particles or more a held step takes the fork / join order of the two streams (as behind any
 * other call on the handle); held == -1 does not. A step that drops itself (a raised flag, found at phd_sync) leaves the old
 * state, the held slot's included. The logs behave as behind phd_step_async. The side buffer (max_components records) is
 * made at the first call with held >= 0.
 * PHD_ERR_BAD_ARGUMENT, with nothing enqueued: a NULL handle, a handle without particles, `held` outside [-1, particles),
 * frozen mode (phd_set_frozen), a multi-device handle, a handle that has run sharded steps.
 * Hosts detect the call by symbol: the API version does not change.                                                        */
int phd_step_hold_async(phd_navigator* nav, int held);
/* Workspace of the set log-likelihood for data-association clusters of 65 .. 256 rows (MurtyPairing, GraphCombinatorics.cs:
 * 241-272, has no size limit; clusters of up to 64 rows work in a per-particle block and never fail): one slab per handle,
 * 128 MiB by default, about 0.4 MB per cluster of 128 rows and 1.3 MB per cluster of 256 in one step. When a step runs out
 * of it (PHD_ERR_ASSOCIATION) the state is kept: raise it here and run the step again.                                */
int phd_set_association_workspace(phd_navigator* nav, int64_t bytes);
/* Benchmark aid: when frozen, a step reads the current state but does not replace it, so every
 * step sees identical input sizes (SURVEY §8d "steady state").                                   */
int phd_set_frozen(phd_navigator* nav, uint8_t frozen);
/* Benchmark mode of SURVEY §8d: every (component, measurement) pair of the correct step is evaluated and the radius gate
 * of Map.Near (PHDNavigator.cs:882) only masks, so that the unit count P x C x M is exact. Off (the default) a group of 64
 * pairs that all lie outside the gate is skipped, as the reference never evaluates them; the results are bit-identical.  */
int phd_set_all_pairs(phd_navigator* nav, uint8_t all_pairs);
/* Scheduling knob (1..4; 0 = chosen from the particle count, the default; environment PHD_SPLIT at phd_create): the per-particle kernels of a
 * step are launched as `nsplit` particle sub-ranges on concurrent streams, forked from and joined into the
 * handle's stream. Results do not depend on it.                                                  */
int phd_set_split(phd_navigator* nav, int nsplit);

/* Getters. Buffers are library-owned and valid until the next call on the handle.               */
const double* phd_weights(phd_navigator* nav, int* length);               /* VehicleWeights       */
int           phd_best_particle(phd_navigator* nav);                       /* BestParticle         */
const double* phd_poses(phd_navigator* nav, int* length);                  /* 7 per particle       */
int           phd_particle_count(phd_navigator* nav);
/* ≙ MapModels[particle] (PHDNavigator.cs:134) / BestMapModel (:155-161): n components,
 * w[n], mean[3n], cov[9n] row-major like isam2.cpp:95-119.                                       */
int phd_map(phd_navigator* nav, int particle, int* ncomp,
            const double** w, const double** mean3, const double** cov9);
/* Source slot of every particle in the last step (identity when no resampling happened); the
 * host applies it to its own per-particle objects (trajectories). `resampled` <- 0/1. It knows the LAST step only: a host
 * that posts steps without waiting for each, or runs the motion model on the device, keeps its trajectories with the
 * trajectory log below instead.                                                                  */
const int32_t* phd_resample_sources(phd_navigator* nav, int* length, uint8_t* resampled);

/* ---- particle trajectories on the device (Vehicle.WayPoints per particle: Vehicle.cs:335, TrackVehicle.cs:101, deep-copied
 * with the vehicle by ResampleParticles, PHDNavigator.cs:740) -------------------------------------------------------------
 * An opt-in log per handle of the particle poses and of who descends from whom, written on the handle's stream without a
 * host wait. Its meaning is the reference's, as a list per particle: an append pushes (i, pose of particle i) onto
 * particle i's list; a step that resampled replaces the lists by new[i] = copy(old[source[i]]). A step that did not
 * resample, a dropped step (PHD_ERR_CAPACITY / PHD_ERR_ASSOCIATION, and the steps queued behind it until phd_sync) and a
 * step in frozen mode (phd_set_frozen) change nothing. Off (the default) a step launches nothing for it.
 *
 * phd_history_enable  `capacity` entries (frames); 0 switches the log off and frees it. Every call restarts the log at
 *                     length 0 (that is also how a host does ResetHistory) and waits for the handle's streams. Memory:
 *                     capacity * max_particles * 60 bytes (7 doubles and one slot per particle and entry) and a few words
 *                     per entry and particle more. A failed allocation is PHD_ERR_DEVICE and leaves the log off. Refused
 *                     with PHD_ERR_BAD_ARGUMENT on a multi-device handle; while the log is on, phd_step_local_async and
 *                     phd_step_global[_device]_async are refused the same way (sharded ancestry is not kept).
 * phd_history_append  one entry: the current particle poses and, for every slot, the slot its particle held in the
 *                     previous entry. Asynchronous like phd_update_motion (enqueued on the handle's stream, the bank of
 *                     the current state is looked up on the device): correct right behind phd_step_async and
 *                     phd_update_motion. `time` is kept on the host. A full log: PHD_ERR_CAPACITY at once, nothing is
 *                     enqueued and the log is as it was (it does not grow in place: enable a larger one). A log that is
 *                     off: PHD_ERR_BAD_ARGUMENT.
 * phd_trajectories    the paths of `nparticles` particles of the CURRENT state (indices into it; out of range:
 *                     PHD_ERR_BAD_ARGUMENT), oldest entry first, resamplings since the last append included:
 *                     *length entries; times[length]; poses7[nparticles][length][7]; slots[nparticles][length], the slot
 *                     the ancestor held at that entry. Library-owned buffers, valid until the next call on the handle.
 *                     Waits for the device. The cost follows the number of entries at which a resampling happened, not
 *                     the length of the path (plus the copy of the path itself).
 * phd_reset and phd_upload_state_soa restart the log (length 0, capacity kept).                                        */
int phd_history_enable(phd_navigator* nav, int capacity);
int phd_history_append(phd_navigator* nav, double time);
int phd_trajectories(phd_navigator* nav, const int32_t* particles, int nparticles, int* length,
                     const double** times, const double** poses7, const int32_t** slots);
/* phd_trajectories_at the paths, up to trajectory-log entry `entry`, of the particles that held `slots[i]` AT that entry:
 *                     shape and conventions are phd_trajectories', *length = entry + 1, and nothing that resampled after the
 *                     entry enters (≙ a copy of WayPoints taken at that frame, as UpdateTrajectory takes one of the best
 *                     particle's: Navigator.cs:258-262). PHD_ERR_BAD_ARGUMENT on a multi-device handle, with the log off,
 *                     for an entry outside [0, length) and for a slot outside [0, particles). Which particle was best at
 *                     that frame is the `best` of the newest map-log entry (below) made before it, or 0 after a reset:
 *                     BestParticle changes in SlamUpdate and reset alone.                                                */
int phd_trajectories_at(phd_navigator* nav, int entry, const int32_t* slots, int nslots, int* length,
                        const double** times, const double** poses7, const int32_t** out_slots);

/* ---- the best map of every frame on the device (Navigator.WayMaps: UpdateMapHistory, Navigator.cs:269-272, at the end of
 * every SlamUpdate, PHDNavigator.cs:361; what maps.out is written from) ----------------------------------------------------
 * An opt-in log per handle of BestMapModel, written on the handle's stream without a host wait: an append stores the best
 * particle's components, their number, BestParticle and its pose as they are behind everything enqueued before it. Which
 * particle is best, where its map lies and how large it is are looked up on the device; the host keeps only `time`. A dropped
 * step changes nothing: the append behind it logs the state before it, which is what the getters report. Off (the default)
 * nothing is launched for it. Independent of the trajectory log: either may be on without the other.
 *
 * phd_map_history_enable  room for `entries` appends and for `components` components in all (80 bytes each; the sum of the
 *                         logged maps' sizes). entries = 0 switches the log off and frees it; a negative number is
 *                         PHD_ERR_BAD_ARGUMENT. Every call restarts the log at length 0 and waits for the handle's streams.
 *                         A failed allocation is PHD_ERR_DEVICE and leaves the log off. Refused with PHD_ERR_BAD_ARGUMENT
 *                         on a multi-device handle and on one that has run sharded steps; while the log is on,
 *                         phd_step_local_async and phd_step_global[_device]_async are refused the same way (the best
 *                         particle may live on another shard).
 * phd_map_history_append  one entry. Asynchronous like phd_history_append (one launch on the handle's stream): correct right
 *                         behind phd_step_async. An entry whose components do not fit what is left of `components` stores
 *                         none and gets the count -1; later entries that fit are stored. A log of `entries` entries:
 *                         PHD_ERR_CAPACITY at once, nothing is enqueued and the log is as it was. A log that is off, a
 *                         handle without particles and frozen mode (phd_set_frozen: BestParticle then describes a result
 *                         the state never took): PHD_ERR_BAD_ARGUMENT.
 * phd_map_history         the log, oldest entry first: *length entries; times, best, counts [length]; best_pose7
 *                         [length][7]; offsets[length + 1], in components, into w / mean3 / cov9 (phd_map's conventions):
 *                         entry k's components are offsets[k] .. offsets[k + 1]. Library-owned buffers, valid until the next
 *                         call on the handle. Waits for the device; one copy of the entry table and one of the components
 *                         in use. If an entry has the count -1 the call returns PHD_ERR_CAPACITY with all outputs set (that
 *                         entry is empty); phd_last_error names the first one.
 * phd_reset and phd_upload_state_soa restart the log (length 0, capacities kept).                                       */
int phd_map_history_enable(phd_navigator* nav, int entries, int64_t components);
int phd_map_history_append(phd_navigator* nav, double time);
int phd_map_history(phd_navigator* nav, int* length, const double** times, const int32_t** best, const double** best_pose7,
                    const int32_t** counts, const int64_t** offsets, const double** w, const double** mean3, const double** cov9);

/* ---- the map error of every logged map (postanalysis: Plot.MapError, Plot.cs:478-529; Plot.OSPA, :531-581) ---------------
 * The reference's map-error time series over the map log above, computed where the maps lie: one workgroup per entry, FP64.
 * (Added without a version bump: hosts detect it by symbol.) For every entry k, in log order:
 *   1. Map.BestMapEstimate (Map.cs:119-142) of the logged components: J = (int) ExpectedSize picks from the list sorted stably
 *      by falling weight, every pick re-entering with its weight less one (a component of weight >= 2 is picked twice);
 *      estimate_size[k] = J. The weights are added in map order wherever a tree sum lies within 1e-9 * max(1, sum) of an integer.
 *   2. where align_pose7 is given and has_reference[k] is not 0 (NULL: all 1), the alignment of Plot.MapError by the estimated
 *      and the true pose at the reference time, align_pose7[k][0] and [k][1] (x y z qw qx qy qz): p' = R(dq*)(p - c) + c - dx
 *      with c the estimated location, exactly as monorfs_amd/host/Ospa.hpp::MapError states it. The poses are the host's input:
 *      it has the estimated one from phd_trajectories_at and the true one from its record.
 *   3. Plot.OSPA between truth3 (ntruth points: the visited map) and the moved estimate with C = cutoff and P = order: with
 *      m <= n the sizes of the two sets, ospa = ((min over assignments of sum min(C, d)^P + C^P (n - m)) / n)^(1/P) and
 *      cardinality = C ((n - m) / n)^(1/P); a pair costs C^P unless C^P - min(C, d)^P > 1e-5 (Plot.cs:561); an empty smaller
 *      set gives C for both, 0 when both sets are empty (:539-542).
 *   4. spatial = (ospa^P - cardinality^P)^(1/P) (:519).
 * times, ospa, cardinality, spatial, estimate_size: [*length], library-owned, valid until the next call on the handle. Waits
 * for the device; the state and both logs are left as they are.
 * One entry handles sets of up to PHD_MAP_ERROR_MAX points each (the kernel keeps both sets and the assignment's row state in
 * 62 KB of LDS, the columns in registers, four per thread). An entry whose J is larger gets NaN values and the size J, an entry
 * that stored no components (count -1) NaN values and the size -1; the call then returns PHD_ERR_CAPACITY with all outputs
 * set, and phd_last_error names the first such entry.
 * PHD_ERR_BAD_ARGUMENT: the map log is off, a multi-device handle, ntruth < 0 or > PHD_MAP_ERROR_MAX, cutoff <= 0,
 * order < 1, non-finite truth3 / align_pose7 / cutoff / order. PHD_ERR_GENERIC: an entry's assignment met its loop bound
 * (possible only with logged records that are no numbers); that entry's values are NaN.                                  */
#define PHD_MAP_ERROR_MAX 1024
int phd_map_error(phd_navigator* nav, const double* truth3, int ntruth, double cutoff, double order,
                  const double* align_pose7,      /* [length][2][7]: estimated, true pose per entry; NULL: no alignment */
                  const uint8_t* has_reference,   /* [length], or NULL = all 1 when align_pose7 is given                */
                  int* length, const double** times, const double** ospa, const double** cardinality,
                  const double** spatial, const int32_t** estimate_size);

/* ---- the pose-error series over the trajectory log (postanalysis: Plot.LocationError, RotationError, OdoLocationError,
 * OdoRotationError, Plot.cs:293-456) ------------------------------------------------------------------------------------------
 * What postanalysis writes as .loc.data, .rot.data, .odoloc.data and .odorot.data, computed where the poses and the ancestry
 * lie: one workgroup per estimate, FP64. (Added without a version bump: hosts detect it by symbol.)
 * Let L be the trajectory log's length. truth7 is the true pose G[k] at every entry (ntruth == L). The estimates are the
 * entries i = first_entry .. L - 1 (a host whose entry 0 is the constructor's waypoint, which no Update copied, passes 1; one
 * that appends only in Update passes 0). E_i is the path of the particle that held slots[i] at entry i: E_i[k], k = 0 .. i, is
 * its ancestor's pose at entry k, exactly what phd_trajectories_at(nav, i, &slots[i], 1, ...) returns.
 * slots == NULL: the estimate at entry k is the `best` of the newest map-log entry appended before trajectory entry k, slot 0
 * if there is none (the rule stated at phd_trajectories_at); the library remembers the map log's length at every
 * phd_history_append and the kernel reads the best particles from the map log's table on the device.
 * With r(k) = min(k, ref_entry), a (-) b = Pose3D.Subtract (Pose3D.cs:297-308), FromLinear = Identity.Add (:247-250, 282-291),
 * every pose read through Pose3D.FromState (the quaternion scaled to norm 1), diffloc(a, b) = |FromLinear(a (-) b).Location|
 * and diffrot(a, b) = |NormalizeAngle(2 acos(W))| of FromLinear(a (-) b).Orientation (Quaternion.cs:71-74, Util.cs:79-87),
 * the per-pose errors of a path E are (Plot.cs:371-456)
 *   loc(E, k)    = diffloc(FromLinear(G[k] (-) G[r(k)]), FromLinear(E[k] (-) E[r(k)])),  rot(E, k) the same with diffrot;
 *   odoloc(E, j), odorot(E, j): j = 0 is the constant 0.0, j >= 1 is diffloc / diffrot of FromLinear(G[k] (-) G[k - 10])
 *                against FromLinear(E[k] (-) E[k - 10]) with k = j + 9: the series has 1 + max(0, |E| - 10) values.
 * The arguments of both acos calls (Quaternion.Log's and Angle's) are clamped to [-1, 1]; the reference returns NaN one ulp
 * above 1. monorfs_amd/host/PoseError.hpp states the same metric sequentially on the host.
 *   PHD_POSE_ERROR_SMOOTH  E = E_{L-1}. location, rotation, times: [L], by entry, times[k] the log's time of entry k. The
 *                          odometry series: 1 + max(0, L - 10) values, odo_times the times of entries 0, 10, 11, ...
 *   PHD_POSE_ERROR_FILTER  E[j] = E_k[k], the pose of slot slots[k] at entry k = first_entry + j itself, against G[k]:
 *                          L - first_entry positions j. The same series over that sequence; ref_entry and the ten of the
 *                          odometry series count positions j; times are those of the entries first_entry + j.
 *   PHD_POSE_ERROR_TIMED   one value per estimate i, in the order of i, times[.] the time of entry i:
 *                          sum_{j = start_i}^{n - 1} series(E_i, j) / (n - start_i), n the series' length for that path
 *                          (i + 1; 1 + max(0, i + 1 - 10) for the odometry series) and start_i the number of estimates
 *                          i' < i whose entry time is < slam_time (Plot.cs:343-362; 0 when there is no "SLAM ... on" tag).
 *                          The division is done as written: an empty range gives 0 / (n - start_i), -0 for a negative count
 *                          and NaN for 0 / 0, which the odometry series do reach and the reference prints.
 *                          odo_length == length, odo_times == times. Each sum is taken as 256 partials (every 256th value
 *                          of the range to one partial, in order) and one fixed tree over them: the same bits on every run.
 * All outputs are library-owned and valid until the next call on the handle. Waits for the device; the state and both logs are
 * left as they are. A refused call leaves every output untouched.
 * One call handles a log of up to PHD_POSE_ERROR_MAX entries of a handle of up to 65 536 particles (the kernel keeps a path's
 * slots in LDS, 16 bits each): PHD_ERR_CAPACITY beyond either, known before anything is enqueued.
 * PHD_ERR_BAD_ARGUMENT: the trajectory log is off or empty, a multi-device handle, ntruth != L, a mode outside 0..2,
 * first_entry outside [0, L), ref_entry < 0, a slot outside [0, particles), non-finite truth7 or slam_time, a truth quaternion
 * of norm 0; with slots == NULL also: the map log is off, or was restarted (phd_map_history_enable, phd_reset,
 * phd_upload_state_soa) since any of the L entries was made.                                                              */
#define PHD_POSE_ERROR_TIMED  0   /* HistMode.Timed  (Plot.cs:340-365) */
#define PHD_POSE_ERROR_SMOOTH 1   /* HistMode.Smooth (:328-329)        */
#define PHD_POSE_ERROR_FILTER 2   /* HistMode.Filter (:331-338)        */
#define PHD_POSE_ERROR_MAX    24576
int phd_pose_error(phd_navigator* nav, int mode,
                   const double* truth7, int ntruth,   /* [ntruth][7]: the true pose at every trajectory-log entry; ntruth == log length */
                   const int32_t* slots,               /* [ntruth]: the slot whose path is the estimate at entry k; NULL: from the map log */
                   int first_entry, int ref_entry, double slam_time,
                   int* length, const double** times, const double** location, const double** rotation,
                   int* odo_length, const double** odo_times, const double** odo_location, const double** odo_rotation);

/* Stage-level entry points for the unit KATs (the stages behind PHDNavigator's public methods).
 *   phd_stage_run(z, with_alpha)  runs predict -> correct -> prune (-> alpha) on EVERY particle of the handle's state, without
 *                                 the weight normalisation / resampling, and leaves each stage's result on the device:
 *   phd_stage_map(stage, particle) reads one particle's mixture after that stage (phd_map's conventions):
 *       PHD_STAGE_PREDICTED  ≙ PredictConditional (PHDNavigator.cs:793-819): state map -> predicted (prior + births)
 *       PHD_STAGE_CORRECTED  ≙ CorrectConditional (:829-906) fused with the MinWeight cut of PruneModel, unsorted
 *                            (the WHOLE list down to MinWeight. A step — phd_slam_update, phd_step_async, phd_step_local_async —
 *                            may emit fewer entries than a stage run: PruneModel keeps only the MaxQuantity heaviest entries,
 *                            so a step leaves out detection updates whose exact weight lies below a floor that MaxQuantity
 *                            entries are certain to reach; the pruned maps and everything behind them are the same bits. A
 *                            step's emitted list is never exposed: only a stage run's is, through this stage.)
 *       PHD_STAGE_PRUNED     ≙ PruneModel (:913-948)
 *   phd_stage_alpha()        ≙ WeightAlpha (:373-393), one value per particle
 *   phd_stage_setloglik()    ≙ SetLogLikelihood (:462-515), one value per particle                                        */
#define PHD_STAGE_PREDICTED 0
#define PHD_STAGE_CORRECTED 1   /* corrected components with weight >= MinWeight, unsorted */
#define PHD_STAGE_PRUNED    2
int phd_stage_run(phd_navigator* nav, const double* z3, int nmeasurements, uint8_t with_alpha);
int phd_stage_map(phd_navigator* nav, int stage, int particle, int* ncomp,
                  const double** w, const double** mean3, const double** cov9);
const double* phd_stage_alpha(phd_navigator* nav, int* length);      /* WeightAlpha per particle  */
const double* phd_stage_setloglik(phd_navigator* nav, int* length);  /* SetLogLikelihood          */

/* ≙ ResampleParticles (:724-760), ParticleDepleted (:768-777) on caller-supplied weights.        */
int phd_resample(phd_navigator* nav, const double* weights, int nparticles, double u_resample,
                 int32_t* sources, int32_t* best_particle);
int phd_particle_depleted(phd_navigator* nav, const double* weights, int nparticles, uint8_t* depleted);

/* ---- multi-GPU (one handle per GPU, particles sharded contiguously) ---------------
 * The step is split around the one exchange the path has (PHDNavigator.cs:343-358):
 *   phd_step_local_async : predict/correct/prune/reweight of the local shard;
 *   the host all-gathers the un-normalised local weights (RCCL over xGMI);
 *   phd_step_global_async: normalise, BestParticle, depletion test and systematic resampling on
 *                          the gathered vector (identical on every rank), local part of the copy;
 * Device pointers are exposed so the collective runs on device memory without staging.          */
int   phd_step_local_async(phd_navigator* nav, uint8_t onlymapping);
void* phd_device_local_weights(phd_navigator* nav);                 /* double[local particles + 1]: an export buffer at a fixed
                                                                       address, filled by phd_step_local_async on the handle's stream —
                                                                       the un-normalised weights and, behind them, the step's status word */
void* phd_device_global_weights(phd_navigator* nav, int world_particles); /* double[world]         */
int   phd_step_global_async(phd_navigator* nav, int rank, int world_size, double u_resample);
/* Particle migration after a global resample: packs the particles other ranks need into a
 * contiguous device buffer (send), and unpacks what arrived (recv). Counts are in particles.
 * The plan is made on the device by phd_step_global_async (at most 64 ranks); phd_migration_plan only waits for its 2 n
 * split sizes, which the plan kernel writes to pinned host memory (no stream synchronisation, no vector crosses).    */
int   phd_migration_plan(phd_navigator* nav, int rank, int world_size,
                         int32_t* send_counts, int32_t* recv_counts);
/* The plan itself, as a pure host function (needs no handle and no GPU): `gsrc[world * Pl]` is the
 * global source vector; send_list (<= Pl * (world - 1) entries) = local indices to pack, grouped by
 * destination rank; dst_code[Pl] = local source index, or -(k + 1) for record k of the receive
 * buffer. Returns the number of received records. A source particle is sent to a rank once for every run of that rank's
 * consecutive slots that take it (its copies share the record, as the copies of a local particle share its map).  */
int   phd_plan_migration(const int32_t* gsrc, int particles_per_rank, int world_size, int rank,
                         int32_t* send_counts, int32_t* recv_counts, int32_t* send_list, int32_t* dst_code);
/* Test surface: the plan as the DEVICE makes it inside a step (k_plan_migration; phd_plan_migration is its host statement and
 * its reference in the tests), on a caller-supplied non-decreasing global source vector. Arrays as phd_plan_migration's, plus
 * fslot[<= particles_per_rank] (the slot each arriving record is unpacked into) and send_dst[<= particles_per_rank + 64][2]
 * (destination rank, record number in that rank's receive buffer). *status: 0 ok, 1 dropped, 2 not a resampling result
 * (decreasing / out of range), 3 send list overflow.                                                                   */
int   phd_test_migration_plan(phd_navigator* nav, const int32_t* gsrc, int particles_per_rank, int world_size, int rank, int resampled,
                              int32_t* send_counts, int32_t* recv_counts, int32_t* send_list, int32_t* dst_code, int32_t* fslot,
                              int32_t* send_dst, int32_t* nsend, int32_t* nrecv, int32_t* status);
/* 1 / 0: the last global step did / did not resample, as phd_migration_plan learnt it (the same on every rank: when it did
 * not, all ranks may skip pack and the all-to-all together; phd_migration_unpack_async still ends the step); -1: not known. */
int   phd_last_resampled(phd_navigator* nav);
void* phd_migration_send_buffer(phd_navigator* nav, int64_t* bytes_per_particle);
void* phd_migration_recv_buffer(phd_navigator* nav);
int   phd_migration_pack_async(phd_navigator* nav);
int   phd_migration_unpack_async(phd_navigator* nav);
/* The sharded step with NOTHING for the host to wait for (round 4; what `bench.py --gpus N` runs). The senders store each
 * migrating particle straight into its place in the receiver's buffer, from the plan the device made; RCCL carries exactly
 * what the north star names, the particle weights:
 *   once      every rank: phd_migration_ipc_export -> 64 bytes (hipIpcMemHandle_t of its receive buffer, fine-grained device
 *             memory); the hosts exchange them; phd_migration_ipc_open(all of them, in rank order). Shards that live in ONE
 *             process hand each other's phd_migration_recv_buffer to phd_migration_set_peers instead.
 *   per step  phd_step_local_async
 *             all-gather of the P + 1 doubles of phd_device_local_weights into phd_device_gather_buffer(world) [world][P + 1]
 *             phd_step_global_device_async   the status words of ALL ranks are read (a flag anywhere drops the step everywhere),
 *                                            global normalise / BestParticle / resampling, the migration plan — on the device
 *             phd_migration_push_async       peer stores of the migrating records
 *             "every rank's records have landed": with phd_migration_set_landing(1) (round 5) the push ends with a store of
 *                                            the step's number into a flag word of every peer's receive buffer and the unpack
 *                                            waits, on the device, for the words of the ranks it takes records from — ONE
 *                                            collective per step, the weights; with the default (0) the caller puts a
 *                                            collective on the same stream here (a one-word all-reduce, rounds 3 - 4)
 *             phd_migration_unpack_async
 * The host never learns whether the step resampled, how many particles moved, or whether a flag dropped it, before phd_sync
 * (which reports a step dropped here because ANOTHER rank raised a flag as PHD_ERR_GENERIC; that rank's own phd_sync names
 * the flag). Results are bit-identical to the host-plan sequence above and to a single handle holding all particles.   */
void* phd_device_gather_buffer(phd_navigator* nav, int world_size);   /* double[world_size][max_particles + 1]; rank r's P + 1 doubles at r * (P + 1) */
int   phd_step_global_device_async(phd_navigator* nav, int rank, int world_size, double u_resample, uint8_t onlymapping);
int   phd_migration_ipc_export(phd_navigator* nav, void* handle64, int64_t* buffer_bytes);
int   phd_migration_ipc_open(phd_navigator* nav, const void* handles /* [world_size][64] */, int rank, int world_size);
int   phd_migration_set_peers(phd_navigator* nav, void* const* recv_buffers /* [world_size], entry `rank` ignored */, int rank, int world_size);
int   phd_migration_recv_is_finegrained(phd_navigator* nav);         /* 1 / 0; -1: no buffer                                         */
int   phd_migration_push_async(phd_navigator* nav);
/* 1: landing flags (needs fine-grained receive buffers: refused with PHD_ERR_BAD_ARGUMENT otherwise); 0: the caller's collective.
 * A flag that does not arrive within 10 s (environment PHD_LANDING_TIMEOUT_MS, read by this call) ends the wait; the next phd_sync
 * reports PHD_ERR_GENERIC (a peer has died; the handle's state is then undefined: phd_reset / upload). The wait is one wave in a
 * launch of its own in front of the unpack kernel: it holds one slot of the device, so ranks may share a GPU.                       */
int   phd_migration_set_landing(phd_navigator* nav, int flags);
void* phd_stream(phd_navigator* nav);                               /* hipStream_t of the handle   */
/* Lend the handle a host stream (hipStream_t, NULL = the default stream): kernels and the host's
 * collectives are then ordered by that stream and need no synchronisation in between;
 * lend = 0 returns to the handle's own stream.                                                   */
int   phd_set_stream(phd_navigator* nav, void* stream, uint8_t lend);

/* SURVEY row f4 (next to the path): PHDNavigator.QuasiSetLogLikelihood (PHDNavigator.cs:526-531) — the set
 * log-likelihood with everything fully visible (constant PD, gate 12) — for a BATCH of candidate poses against one
 * landmark set and one measurement set: the shape of the smoother's pose searches (LoopyPHDNavigator.cs:777-909).
 * poses7[nposes][7], landmarks3[nlandmarks][3], z3[nmeasurements][3]; out[nposes]. nposes <= max_particles,
 * nlandmarks <= min(1024, max_quantity rounded up to a multiple of 64): the landmark scratch of a step's map estimate
 * (an estimate beyond it is PHD_ERR_CAPACITY there); more landmarks are PHD_ERR_BAD_ARGUMENT. Synchronous; does not
 * touch the particle state.                                                                                       */
int phd_quasi_set_loglik(phd_navigator* nav, const double* poses7, int nposes, const double* landmarks3, int nlandmarks,
                         const double* z3, int nmeasurements, double* out);

/* The same with the pose gradient: QuasiSetLogLikelihood(measurements, map, pose, out gradient) (PHDNavigator.cs:543-548,
 * calcgradient branches of :556-713) — what LoopyPHDNavigator.LogLikeGradientAscent (:916-965) and LogLikeFitCovariance
 * (:976-1021) call. gradients6[nposes][6]: d/d(translation, rotation) as MeasurementJacobianP (PRM3DMeasurer.cs:185-211)
 * defines them. Every component is enumerated in the reference's order because TemperedAverage (MatrixExtensions.cs:
 * 400-440) rewrites the shared logcomp array in place; in this mode the value can differ from phd_quasi_set_loglik's
 * where a component of more than 5 rows meets those rewritten entries in the cut of :672 — as in the reference.
 * average_mode 0: TemperedAverage as its source reads (weights.Normalize() = division by the Euclidean norm of the whole
 * 200-entry array, Accord.Math 3.0.2, not in the reference tree); 1: weights divided by their sum (the only one of the
 * two under which the reference's own LoopyPHDNavigatorTest.LogLike2D assertion holds; tests/test_oracle_kat.py).     */
int phd_quasi_set_loglik_grad(phd_navigator* nav, const double* poses7, int nposes, const double* landmarks3, int nlandmarks,
                              const double* z3, int nmeasurements, int average_mode, double* out, double* gradients6);

/* LoopyPHDNavigator.LogLikeGradientAscent (LoopyPHDNavigator.cs:916-965) resident on the device, for nestimates initial
 * estimates side by side (monorfs_amd/csrc/phd_ascent.h): what monorfs_amd/loopy.py::LogLikeGradientAscent drives from the
 * host with two batch calls per iteration, as ONE call — one copy in, a chain of kernels, one copy out. Per estimate the
 * reference's loop: the gradient of phd_quasi_set_loglik_grad at the last TRIED pose, clipped to norm 10, the step 1e-2
 * halved up to PHD_ASCENT_LINE times until the value of phd_quasi_set_loglik does not decrease, until an iteration gains no
 * more than 1e-3. The evaluations are the two batch calls' kernels, same bits; an estimate that has stopped is skipped by
 * every later kernel.
 * initial6[nestimates][6] linear poses around linearpoint7 (Pose3D.Add), landmarks3 / z3 / average_mode as for the batch
 * calls. PHD_ASCENT_LINE * nestimates <= max_particles (a line search is one batch): more is PHD_ERR_BAD_ARGUMENT, the
 * wrappers split the estimates into several calls.
 * Iterations are enqueued round_iterations at a time (0: the library's default); between two rounds the host reads one
 * word, the number of estimates still climbing, and stops at zero. The results do not depend on round_iterations.
 * max_iterations >= 1 bounds the call (the reference's loop has no bound): estimates still climbing then return their state
 * after exactly max_iterations iterations and the call returns PHD_ERR_CAPACITY with all outputs set.
 * poses6[nestimates][6], values[nestimates] (the value at poses6), iterations[nestimates] (line searches run).
 * hessians36: NULL, or [nestimates][6][6] row-major — the rows (g(pose + eps e_i) - g(pose - eps e_i)) / (2 eps), eps =
 * 1e-5, of LogLikeFitCovariance (:976-1021) at the returned poses, raw: the NaN test, the eigenvalue clip and the
 * pseudo-inverse stay with the host.
 * PHD_FLAG_BIG_CLUSTER in any evaluation: PHD_ERR_ASSOCIATION. Non-finite input: PHD_ERR_BAD_ARGUMENT. Synchronous; touches
 * neither the particle state nor the logs nor the batch calls' buffers; a multi-device handle uses its first shard.       */
#define PHD_ASCENT_LINE 16
int phd_quasi_ascent(phd_navigator* nav, const double* initial6, int nestimates, const double* linearpoint7,
                     const double* landmarks3, int nlandmarks, const double* z3, int nmeasurements,
                     int average_mode, int max_iterations, int round_iterations,
                     double* poses6, double* values, int32_t* iterations,
                     double* hessians36 /* [nestimates][6][6] row-major, or NULL */);

/* Pose searches of many frames in one call (monorfs_amd/csrc/phd_ascent_multi.h): the GuidedFitMixture of every frame of
 * LoopyPHDNavigator.UpdateMessagesFromMap (:525-551) shares the launches of ONE chain. A PROBLEM is what differs between
 * frames: a landmark set, a measurement set, a linearisation pose. Problem q has the landmarks landmarks3[landmark_offsets[q]
 * .. landmark_offsets[q + 1]), the measurements z3[measurement_offsets[q] .. measurement_offsets[q + 1]) (both offset arrays
 * [nproblems + 1], starting at 0, never decreasing) and linearpoints7[q]. Estimate e starts at initial6[e] and belongs to
 * problem[e]; the estimates of a problem may sit anywhere, a problem may have none.
 * For every estimate the outputs are bit for bit what phd_quasi_ascent returns for it when called with its problem alone at
 * the same average_mode, max_iterations and round_iterations.
 * Limits: PHD_ASCENT_LINE * nestimates <= max_particles; per problem landmarks <= min(1024, max_quantity rounded up to 64)
 * and measurements <= min(max_measurements, 256); the measurement counts of ONE call lie in one block class — all in 0..64,
 * all in 65..128 or all in 129..256, 0 fits any — (the wrappers split a mixed set). Everything is checked before anything
 * is enqueued: a NULL handle or array, nproblems < 1, bad offsets, a problem index outside [0, nproblems), a limit, mixed
 * classes, average_mode not 0 / 1, max_iterations < 1, round_iterations < 0 or non-finite input is PHD_ERR_BAD_ARGUMENT
 * with the outputs untouched. PHD_ERR_ASSOCIATION and PHD_ERR_CAPACITY are call-wide, as for phd_quasi_ascent.
 * Synchronous; a buffer of its own per handle (it grows to the largest call): the particle state, the logs, the step's and
 * the single calls' flag words and slab counters are not touched; a multi-device handle uses its first shard.           */
int phd_quasi_ascent_multi(phd_navigator* nav, int nproblems,
                           const int32_t* landmark_offsets, const double* landmarks3,
                           const int32_t* measurement_offsets, const double* z3,
                           const double* linearpoints7 /* [nproblems][7] */,
                           const double* initial6, const int32_t* problem, int nestimates,
                           int average_mode, int max_iterations, int round_iterations,
                           double* poses6, double* values, int32_t* iterations,
                           double* hessians36 /* [nestimates][6][6] row-major, or NULL */);

/* phd_quasi_set_loglik (gradients6 NULL: the value kernel, average_mode is not read beyond its range check) or
 * phd_quasi_set_loglik_grad for poses of many problems in one launch: pose i is evaluated against problem[i], bit for bit
 * as the single call with that problem alone. nposes <= max_particles; problems, limits and refusals as above.          */
int phd_quasi_set_loglik_multi(phd_navigator* nav, int nproblems,
                               const int32_t* landmark_offsets, const double* landmarks3,
                               const int32_t* measurement_offsets, const double* z3,
                               const double* poses7, const int32_t* problem, int nposes,
                               int average_mode, double* out, double* gradients6 /* or NULL */);

/* The starting guesses of the pose searches of many frames (monorfs_amd/csrc/phd_guesses.h): the guess loop of
 * LoopyPHDNavigator.GuidedFitMixture (:789-797) for every problem of a call, and the first evaluation of every guess
 * (:808-823). Problems as for phd_quasi_ascent_multi — the same offsets arrays, limits and one-block-class rule —, each with
 * its linearisation pose linearpoints7[q] and its initial linear pose pose0s6[q]; initpose = linearpoint.Add(pose0).
 * The guesses of problem q stand at guess_offsets[q] .. guess_offsets[q + 1] in the reference's order: pose0s6[q] itself
 * (pairs2 = -1, -1), then, landmark-major and measurement-minor, every (landmark, measurement) pair whose fitted pose g
 * (PRM3DMeasurer.FitToMeasurement at initpose, PRM3DMeasurer.cs:221-243) has |g.Subtract(initpose)|^2 < radius^2 (0.5 in
 * the reference, :793), stored as g.Subtract(linearpoint). A pair whose fit is not finite (a landmark at the pose's
 * location, a landmark direction exactly opposite the measurement's) makes no guess: the comparison is false on NaN.
 * pairs2[e] = (landmark, measurement), problem-local. poses7[e] = linearpoint.Add(guesses6[e]), the pose a search forms from
 * the same guess; values[e] is bit for bit what phd_quasi_set_loglik_multi returns for poses7[e], emptyspace[q] what it
 * returns for farpose7 (the pose far from everything, :808) against problem q. The evaluations run inside the call, at most
 * max_particles poses a launch.
 * capacity: the guesses pairs2 / guesses6 / poses7 / values hold. More guesses than that: PHD_ERR_CAPACITY with guess_offsets
 * fully set (guess_offsets[nproblems] is the capacity a retry needs) and every other output untouched. capacity < nproblems,
 * a radius that is not finite and > 0, a NULL handle or array, bad offsets, a limit, mixed classes or non-finite input:
 * PHD_ERR_BAD_ARGUMENT before anything is enqueued, the outputs untouched. PHD_FLAG_BIG_CLUSTER in any evaluation:
 * PHD_ERR_ASSOCIATION. Synchronous; buffers of its own per handle: the particle state, the logs and the other calls' flag
 * words and slab counters are not touched; a multi-device handle uses its first shard.                                  */
int phd_quasi_guesses_multi(phd_navigator* nav, int nproblems,
                            const int32_t* landmark_offsets, const double* landmarks3,
                            const int32_t* measurement_offsets, const double* z3,
                            const double* linearpoints7 /* [nproblems][7] */,
                            const double* pose0s6 /* [nproblems][6] */,
                            const double* farpose7 /* [7] */, double radius, int capacity,
                            int32_t* guess_offsets /* [nproblems + 1] */,
                            int32_t* pairs2 /* [capacity][2] */,
                            double* guesses6 /* [capacity][6] */, double* poses7 /* [capacity][7] */,
                            double* values /* [capacity] */, double* emptyspace /* [nproblems] */);

/* Test surface for the control kernels of phd_quasi_ascent: k_ascent_candidates, then k_ascent_select on the caller's
 * values16[nestimates][16], no evaluation in between, every estimate active. Returns cand6[n][16][6], cand7[n][16][7], the
 * index of the candidate the line search ended on, the new pose6 / loglike, nextpose7 and the active word.              */
int phd_test_ascent_control(phd_navigator* nav, const double* pose6, const double* loglike, const double* gradients6, const double* values16,
                            int nestimates, const double* linearpoint7, double* cand6, double* cand7, int32_t* chosen,
                            double* newpose6, double* newloglike, double* nextpose7, int32_t* active);

/* Test surface for the assignment enumerators the set log-likelihood runs on the device: MurtyPairing (mode 0,
 * GraphCombinatorics.cs:241-272; n <= 256) or LexicographicalPairing(matrix, modelsize) (mode 1, :280-334; n <= 5) on a
 * dense n x n profit matrix (row-major, -inf = no entry). assignments[k][n] (row -> column; -1: an unsolved first node),
 * values[k] for the first min(count, maxcount) pairings in the order they are produced; *count = how many there are
 * (at most 200, the length of the reference's logcomp). The vectors of GraphCombinatoricsTest.cs go through this.  */
int phd_test_pairing(phd_navigator* nav, const double* matrix, int n, int mode, int modelsize, int maxcount,
                     int32_t* assignments, double* values, int* count);

/* Test surface for the device arithmetic primitives (exp_neg / exp_pair and their table, gauss_record / gauss_logw, the
 * double-double helpers of the resampling, small_div, the weight bins, the fixed-order reductions and scans, the 3 x 3
 * algebra): k_test_primitive calls the function `op` names on every record of `in` and writes the records of `out`. Both
 * are raw bytes in the layout monorfs_amd/csrc/phd_primitives_test.h documents per op, so that bit patterns pass
 * unchanged. PHD_ERR_BAD_ARGUMENT for an unknown op or sizes that do not match its layout. A multi-device handle runs
 * it on its first shard. tests/test_gpu_primitives.py holds each primitive to a multi-precision reference through it.   */
int phd_test_primitive(phd_navigator* nav, int op, const void* in, int64_t in_bytes, void* out, int64_t out_bytes);

/* Per-kernel device time in milliseconds, from HIP events recorded around every launch on the
 * handle's stream: the mean over the launches since the last phd_timing_reset; names[i] -> ms[i];
 * returns the number of entries. phd_timing_reset(nav, 0) switches the events off; (nav, n) times every n-th
 * step only (an event costs the device a few microseconds).                                      */
int phd_timing_reset(phd_navigator* nav, uint8_t enabled);
int phd_last_timings(phd_navigator* nav, const char*** names, const double** ms);
/* Launches behind each mean of the last phd_last_timings call, same order (a split step launches a kernel
 * once per particle sub-range).                                                                  */
int phd_last_timing_counts(phd_navigator* nav, const int** counts);

/* Bulk upload / download of the whole particle set (benchmark and tests), host arrays plane per field:
 * planes[10][nparticles][stride] = w, mean x y z, covariance xx xy xz yy yz zz; counts[nparticles];
 * poses7[nparticles][7]; weights[nparticles]. (The device keeps ONE 80-byte record per component — w, mean, covariance
 * upper triangle —, [particle][slot][10]: the conversion happens here, at the edge; only the first counts[i] slots of a
 * particle are read / written.) The upload sets the particle count; the download gathers the maps of a resampled state
 * into place first (see phd_set_map).                                                            */
int phd_upload_state_soa(phd_navigator* nav, int nparticles, int stride, const double* planes,
                         const int32_t* counts, const double* poses7, const double* weights);
int phd_download_state_soa(phd_navigator* nav, int stride, double* planes, int32_t* counts,
                           double* poses7, double* weights);

#ifdef __cplusplus
}
#endif
#endif /* PHDHIP_H */
