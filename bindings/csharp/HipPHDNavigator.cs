// HipPHDNavigator.cs — the reference-side binding a monorfs maintainer would add next to
// mono-rfs-lib/SLAM/Navigators/PHDNavigator.cs to run the PHD inner loop on an MI355X.
//
// NOT COMPILED HERE: this image has no mono/mcs/dotnet (SURVEY.md §8c). It follows, member by member,
// the one native binding the reference already ships (ISAM2Lib, ISAM2Navigator.cs:600-622):
// DllImport on a non-generic static class, HandleRef for the opaque navigator, `fixed` pinning of the
// caller-owned arrays for the duration of a call, library-owned result buffers copied out with
// Marshal.Copy, bool as UnmanagedType.U1, and a non-zero status turned into an
// InvalidOperationException carrying Data["module"] (ISAM2Navigator.cs:239-262), which
// Simulation.Update already catches (Simulation.cs:655-670).
//
// Wiring: add `case NavigationAlgorithm.HipPHD: navigator = new HipPHDNavigator(explorer, particlecount, onlymapping);`
// to the switch in Simulation.FromFiles (Simulation.cs:352-379) and the option value to Program.cs:119.
using System;
using System.Collections.Generic;
using System.Runtime.InteropServices;

using Microsoft.Xna.Framework;

namespace monorfs
{
[StructLayout(LayoutKind.Sequential)]
public unsafe struct PhdParams          // include/phdhip.h: struct phd_params
{
	public int model, zdim;
	public fixed double measurer[7];
	public fixed double R[9];
	public fixed double visibility_ramp[3];
	public double pd, clutter_density;
	public fixed double birth_covariance[9];
	public double birth_weight, min_weight, min_effective_particle;
	public int max_quantity, gate_metric;
	public double merge_threshold, exploration_threshold, density_distance_threshold;
	public int max_particles, max_components, max_measurements, emit_capacity;
}

public class PhdHipLib
{
	const string Lib = "libphdhip.so";
	[DllImport(Lib)] public extern static IntPtr phd_create(ref PhdParams p, int device);
	[DllImport(Lib)] public extern static IntPtr phd_create_multi(ref PhdParams p, int[] devices, int ndevices);
	[DllImport(Lib)] public extern static int    phd_multi_report(HandleRef nav, double[] out9, byte[] p2p, out int nshards);
	[DllImport(Lib)] public extern static IntPtr phd_create_error();
	[DllImport(Lib)] public extern static void   phd_destroy(HandleRef nav);
	[DllImport(Lib)] public extern static IntPtr phd_last_error(HandleRef nav);
	[DllImport(Lib)] public extern static int    phd_reset(HandleRef nav, int nparticles, IntPtr pose7, IntPtr w, IntPtr mean3, IntPtr cov9, int ncomp);
	[DllImport(Lib)] public extern static int    phd_set_poses(HandleRef nav, IntPtr poses7, int nparticles);
	[DllImport(Lib)] public extern static int    phd_update_motion(HandleRef nav, IntPtr odometry6, IntPtr noise6, int nparticles, [MarshalAs(UnmanagedType.U1)] bool perfectstill);
	[DllImport(Lib)] public extern static int    phd_quasi_set_loglik_grad(HandleRef nav, IntPtr poses7, int nposes, IntPtr landmarks3, int nlandmarks, IntPtr z3, int nmeasurements, int averagemode, IntPtr result, IntPtr gradients6);
	[DllImport(Lib)] public extern static int    phd_quasi_set_loglik(HandleRef nav, IntPtr poses7, int nposes, IntPtr landmarks3, int nlandmarks, IntPtr z3, int nmeasurements, IntPtr result);
	[DllImport(Lib)] public extern static int    phd_quasi_ascent(HandleRef nav, IntPtr initial6, int nestimates, IntPtr linearpoint7, IntPtr landmarks3, int nlandmarks, IntPtr z3, int nmeasurements, int averagemode, int maxiterations, int rounditerations, IntPtr poses6, IntPtr values, IntPtr iterations, IntPtr hessians36);
	[DllImport(Lib)] public extern static int    phd_quasi_ascent_multi(HandleRef nav, int nproblems, IntPtr landmarkoffsets, IntPtr landmarks3, IntPtr measurementoffsets, IntPtr z3, IntPtr linearpoints7, IntPtr initial6, IntPtr problem, int nestimates, int averagemode, int maxiterations, int rounditerations, IntPtr poses6, IntPtr values, IntPtr iterations, IntPtr hessians36);
	[DllImport(Lib)] public extern static int    phd_quasi_set_loglik_multi(HandleRef nav, int nproblems, IntPtr landmarkoffsets, IntPtr landmarks3, IntPtr measurementoffsets, IntPtr z3, IntPtr poses7, IntPtr problem, int nposes, int averagemode, IntPtr values, IntPtr gradients6);
	[DllImport(Lib)] public extern static int    phd_quasi_guesses_multi(HandleRef nav, int nproblems, IntPtr landmarkoffsets, IntPtr landmarks3, IntPtr measurementoffsets, IntPtr z3, IntPtr linearpoints7, IntPtr pose0s6, IntPtr farpose7, double radius, int capacity, IntPtr guessoffsets, IntPtr pairs2, IntPtr guesses6, IntPtr poses7, IntPtr values, IntPtr emptyspace);
	[DllImport(Lib)] public extern static int    phd_set_depth_map(HandleRef nav, IntPtr depth, int width, int height);
	[DllImport(Lib)] public extern static int    phd_slam_update(HandleRef nav, IntPtr z3, int nmeasurements, [MarshalAs(UnmanagedType.U1)] bool onlymapping, double uresample);
	[DllImport(Lib)] public extern static int    phd_set_measurements(HandleRef nav, IntPtr z3, int nmeasurements);
	[DllImport(Lib)] public extern static int    phd_step_hold_async(HandleRef nav, int held);
	[DllImport(Lib)] public extern static int    phd_sync(HandleRef nav);
	[DllImport(Lib)] public extern static IntPtr phd_weights(HandleRef nav, out int length);
	[DllImport(Lib)] public extern static int    phd_best_particle(HandleRef nav);
	[DllImport(Lib)] public extern static IntPtr phd_poses(HandleRef nav, out int length);
	[DllImport(Lib)] public extern static int    phd_map(HandleRef nav, int particle, out int ncomp, out IntPtr w, out IntPtr mean3, out IntPtr cov9);
	[DllImport(Lib)] public extern static IntPtr phd_resample_sources(HandleRef nav, out int length, [MarshalAs(UnmanagedType.U1)] out bool resampled);
	[DllImport(Lib)] public extern static int    phd_history_enable(HandleRef nav, int capacity);
	[DllImport(Lib)] public extern static int    phd_history_append(HandleRef nav, double time);
	[DllImport(Lib)] public extern static int    phd_trajectories(HandleRef nav, int[] particles, int nparticles, out int length, out IntPtr times, out IntPtr poses7, out IntPtr slots);
	[DllImport(Lib)] public extern static int    phd_trajectories_at(HandleRef nav, int entry, int[] slots, int nslots, out int length, out IntPtr times, out IntPtr poses7, out IntPtr outslots);
	[DllImport(Lib)] public extern static int    phd_map_history_enable(HandleRef nav, int entries, long components);
	[DllImport(Lib)] public extern static int    phd_map_history_append(HandleRef nav, double time);
	[DllImport(Lib)] public extern static int    phd_map_history(HandleRef nav, out int length, out IntPtr times, out IntPtr best, out IntPtr bestpose7, out IntPtr counts, out IntPtr offsets,
	                                                              out IntPtr w, out IntPtr mean3, out IntPtr cov9);
	[DllImport(Lib)] public extern static int    phd_map_error(HandleRef nav, IntPtr truth3, int ntruth, double cutoff, double order, IntPtr alignpose7, IntPtr hasreference,
	                                                            out int length, out IntPtr times, out IntPtr ospa, out IntPtr cardinality, out IntPtr spatial, out IntPtr estimatesize);
	[DllImport(Lib)] public extern static int    phd_pose_error(HandleRef nav, int mode, IntPtr truth7, int ntruth, IntPtr slots, int firstentry, int refentry, double slamtime,
	                                                             out int length, out IntPtr times, out IntPtr location, out IntPtr rotation,
	                                                             out int odolength, out IntPtr odotimes, out IntPtr odolocation, out IntPtr odorotation);
}

/// <summary>
/// PHD SLAM solver running PHDNavigator.SlamUpdate on the GPU. The motion model, its random
/// generators and every per-particle object (TrackVehicle, trajectories) stay in managed code.
/// </summary>
public unsafe class HipPHDNavigatorCore<MeasurerT> : Navigator<MeasurerT, Pose3D, PixelRangeMeasurement>
	where MeasurerT : PRM3DMeasurer, IMeasurer<MeasurerT, Pose3D, PixelRangeMeasurement>, new()
{
	protected HandleRef nav;
	public int ParticleCount { get; set; }
	public TrackVehicle<MeasurerT, Pose3D, PixelRangeMeasurement>[] VehicleParticles { get; private set; }
	public double[] VehicleWeights { get; private set; }
	public int BestParticle { get; private set; }

	/// <summary>gpus: how many GPUs of the node the particles are sharded over (devices 0 .. gpus - 1, one handle, this
	/// thread: phd_create_multi); particlecount must then be a multiple of it. 1, or a mapping-only navigator (one particle):
	/// a single-device handle.</summary>
	public HipPHDNavigatorCore(Vehicle<MeasurerT, Pose3D, PixelRangeMeasurement> vehicle, int particlecount, bool onlymapping = false, int gpus = 1)
		: base(vehicle, onlymapping)
	{
		ParticleCount = particlecount;
		PhdParams p = new PhdParams();
		p.model = 1; p.zdim = 3;
		double[] m = vehicle.Measurer.ToLinear();                         // PRM3DMeasurer.cs:92-96
		for (int i = 0; i < 7; i++) p.measurer[i] = m[i];
		double[][] R = Config.MeasurementCovarianceMultiplier.Multiply(vehicle.MeasurementCovariance);
		for (int i = 0; i < 9; i++) { p.R[i] = R[i / 3][i % 3]; p.birth_covariance[i] = Config.BirthCovariance[i / 3][i % 3]; }
		for (int i = 0; i < 3; i++) p.visibility_ramp[i] = Config.VisibilityRamp[i];
		p.pd = Config.NavigatorPD; p.clutter_density = Config.NavigatorClutterDensity;
		p.birth_weight = Config.BirthWeight; p.min_weight = Config.MinWeight;
		p.min_effective_particle = Config.MinEffectiveParticle; p.max_quantity = Config.MaxQuantity;
		p.gate_metric = 1;                                                // Accord 3.0.x KDTree: squared Euclidean
		p.merge_threshold = Config.MergeThreshold; p.exploration_threshold = Config.ExplorationThreshold;
		p.density_distance_threshold = Config.DensityDistanceThreshold;
		p.max_particles = particlecount; p.max_components = Math.Max(Config.MaxQuantity, 640); p.max_measurements = 256;
		AdjustParams(ref p, vehicle);
		int[] devices = new int[Math.Max(gpus, 1)];
		for (int i = 0; i < devices.Length; i++) devices[i] = i;
		IntPtr h = (gpus > 1 && !onlymapping) ? PhdHipLib.phd_create_multi(ref p, devices, devices.Length) : PhdHipLib.phd_create(ref p, 0);
		if (h == IntPtr.Zero) { throw Fail(Marshal.PtrToStringAnsi(PhdHipLib.phd_create_error()), -1); }
		nav = new HandleRef(this, h);
		reset(RefVehicle, new double[0], new double[0], new double[0], onlymapping ? 1 : particlecount);
	}

	/// <summary>The particles' measurer where it is not the explorer's (HipKinectPHDNavigator: the inflated film).</summary>
	protected virtual void AdjustParams(ref PhdParams p, Vehicle<MeasurerT, Pose3D, PixelRangeMeasurement> vehicle) { }

	/// <summary>Inputs of the coming step besides the measurements (HipKinectPHDNavigator: the depth frame).</summary>
	protected virtual void BeforeSlamUpdate() { }

	protected Exception Fail(string message, int status)
	{
		var e = new InvalidOperationException(message);
		e.Data["module"] = (status == 3) ? "association" : "phdhip";     // Simulation.cs:662-670
		return e;
	}

	protected void Check(int status)
	{
		if (status != 0) { throw Fail(Marshal.PtrToStringAnsi(PhdHipLib.phd_last_error(nav)), status); }
	}

	void reset(Vehicle<MeasurerT, Pose3D, PixelRangeMeasurement> vehicle, double[] w, double[] mean, double[] cov, int particlecount)
	{
		double[] pose = vehicle.Pose.State;
		fixed (double* pp = pose) fixed (double* pw = w) fixed (double* pm = mean) fixed (double* pc = cov) {
			Check(PhdHipLib.phd_reset(nav, particlecount, (IntPtr) pp, (IntPtr) pw, (IntPtr) pm, (IntPtr) pc, w.Length));
		}
		VehicleParticles = new TrackVehicle<MeasurerT, Pose3D, PixelRangeMeasurement>[particlecount];
		for (int i = 0; i < particlecount; i++) {
			VehicleParticles[i] = vehicle.TrackClone(Config.MotionCovarianceMultiplier, Config.MeasurementCovarianceMultiplier,
			                                         Config.NavigatorPD, Config.NavigatorClutterDensity, true);
		}
		VehicleWeights = new double[particlecount];
		for (int i = 0; i < particlecount; i++) { VehicleWeights[i] = 1.0 / particlecount; }
		BestParticle = 0;
	}

	public override TrackVehicle<MeasurerT, Pose3D, PixelRangeMeasurement> BestEstimate { get { return VehicleParticles[BestParticle]; } }

	public override Map BestMapModel
	{
		get {
			int n; IntPtr w, m, c;
			Check(PhdHipLib.phd_map(nav, BestParticle, out n, out w, out m, out c));
			double[] ws = new double[n], ms = new double[3 * n], cs = new double[9 * n];
			if (n > 0) { Marshal.Copy(w, ws, 0, n); Marshal.Copy(m, ms, 0, 3 * n); Marshal.Copy(c, cs, 0, 9 * n); }
			Map map = new Map(3);
			for (int i = 0; i < n; i++) {
				double[][] cov = { new double[] {cs[9*i], cs[9*i+1], cs[9*i+2]}, new double[] {cs[9*i+3], cs[9*i+4], cs[9*i+5]}, new double[] {cs[9*i+6], cs[9*i+7], cs[9*i+8]} };
				map.Add(new Gaussian(new double[] {ms[3*i], ms[3*i+1], ms[3*i+2]}, cov, ws[i]));
			}
			return map;
		}
	}

	public override void ResetMapModel()
	{
		reset(RefVehicle, new double[0], new double[0], new double[0], VehicleParticles.Length);
	}

	/// <summary>Motion update: stays managed (TrackVehicle.UpdateNoisy, PHDNavigator.cs:295-314), then the poses go to the device.</summary>
	public override void Update(GameTime time, double[] reading)
	{
		if (OnlyMapping) { VehicleParticles[0].Pose = RefVehicle.Pose.DClone(); }
		else { for (int i = 0; i < VehicleParticles.Length; i++) { VehicleParticles[i].UpdateNoisy(time, reading); } }
		double[] poses = new double[7 * VehicleParticles.Length];
		for (int i = 0; i < VehicleParticles.Length; i++) { VehicleParticles[i].Pose.State.CopyTo(poses, 7 * i); }
		fixed (double* pp = poses) { Check(PhdHipLib.phd_set_poses(nav, (IntPtr) pp, VehicleParticles.Length)); }
		UpdateTrajectory(time);
	}

	/// <summary>Alternative to Update with the motion step on the device (phd_update_motion): only the reading and the
	/// noise vectors drawn here cross the boundary; the managed particles are refreshed from phd_poses when needed.</summary>
	public void UpdateOnDevice(GameTime time, double[] reading)
	{
		int      n     = VehicleParticles.Length;
		double[] noise = new double[6 * n];
		double   dt    = time.ElapsedGameTime.TotalSeconds;
		for (int i = 0; i < n; i++) {
			double[] v = dt.Multiply(Util.RandomGaussianVector(new double[6], VehicleParticles[i].MotionCovariance));   // TrackVehicle.cs:95-97
			v.CopyTo(noise, 6 * i);
		}
		fixed (double* pr = reading) fixed (double* pn = noise) {
			Check(PhdHipLib.phd_update_motion(nav, (IntPtr) pr, OnlyMapping ? IntPtr.Zero : (IntPtr) pn, n, SimulatedVehicle<MeasurerT, Pose3D, PixelRangeMeasurement>.PerfectStill));
		}
		// the managed particles' WayPoints are not touched on this path: the device keeps the paths (EnableDeviceHistory)
		if (DeviceHistory) { Check(PhdHipLib.phd_history_append(nav, time.TotalGameTime.TotalSeconds)); }
		UpdateTrajectory(time);
	}

	/// <summary>True while the device keeps the particles' paths (EnableDeviceHistory).</summary>
	public bool DeviceHistory { get; private set; }

	/// <summary>The trajectory log on the device (phd_history_enable): room for `capacity` frames, 0 switches it off. Every call
	/// restarts it at length 0, as does every reset (ResetHistory). Single-device handles only.</summary>
	public void EnableDeviceHistory(int capacity)
	{
		Check(PhdHipLib.phd_history_enable(nav, capacity));
		DeviceHistory = capacity > 0;
	}

	/// <summary>≙ VehicleParticles[particle].WayPoints (Vehicle.cs:141) as the device kept it: the path of that particle of the
	/// current state through every resampling, oldest entry first (phd_trajectories; waits for the device). With UpdateOnDevice
	/// this is what Navigator.UpdateTrajectory (Navigator.cs:258-262) should copy for BestParticle.</summary>
	public List<Tuple<double, double[]>> DeviceWayPoints(int particle)
	{
		int length; IntPtr times, poses, slots;
		Check(PhdHipLib.phd_trajectories(nav, new int[] {particle}, 1, out length, out times, out poses, out slots));
		return ToWay(length, times, poses);
	}

	/// <summary>DeviceWayPoints as it was at trajectory-log entry `entry`, for the particle that held `slot` then: entry + 1
	/// entries, nothing that resampled later enters (phd_trajectories_at; waits for the device). A host that posted its frames
	/// without waiting rebuilds UpdateTrajectory's copies from this: the best particle at the Update of a frame is the Best of
	/// the newest DeviceWayMaps entry before it, or 0 after a reset.</summary>
	public List<Tuple<double, double[]>> DeviceWayPointsAt(int entry, int slot)
	{
		int length; IntPtr times, poses, slots;
		Check(PhdHipLib.phd_trajectories_at(nav, entry, new int[] {slot}, 1, out length, out times, out poses, out slots));
		return ToWay(length, times, poses);
	}

	static List<Tuple<double, double[]>> ToWay(int length, IntPtr times, IntPtr poses)
	{
		double[] t = new double[length], x = new double[7 * length];
		if (length > 0) { Marshal.Copy(times, t, 0, length); Marshal.Copy(poses, x, 0, 7 * length); }
		var way = new List<Tuple<double, double[]>>(length);               // TimedState
		for (int k = 0; k < length; k++) {
			double[] state = new double[7];
			Array.Copy(x, 7 * k, state, 0, 7);
			way.Add(Tuple.Create(t[k], state));
		}
		return way;
	}

	/// <summary>True while the device keeps the best map of every frame (EnableDeviceMapHistory).</summary>
	public bool DeviceMapHistory { get; private set; }

	/// <summary>The map log on the device (phd_map_history_enable): room for `entries` frames and `components` components over all
	/// of them, entries = 0 switches it off. Every call restarts it, as does every reset. Single-device handles only.</summary>
	public void EnableDeviceMapHistory(int entries, long components)
	{
		Check(PhdHipLib.phd_map_history_enable(nav, entries, components));
		DeviceMapHistory = entries > 0;
	}

	/// <summary>One entry of the map log: the best particle's map, slot and pose as they are behind everything posted so far
	/// (phd_map_history_append; asynchronous: correct right behind phd_step_async). ≙ UpdateMapHistory (Navigator.cs:269-272)
	/// for a host that does not wait for its steps.</summary>
	public void AppendDeviceMapHistory(GameTime time)
	{
		Check(PhdHipLib.phd_map_history_append(nav, time.TotalGameTime.TotalSeconds));
	}

	/// <summary>≙ WayMaps (Navigator.cs:269-272) as the device kept it, with the best particle and its pose beside every map,
	/// oldest entry first (phd_map_history; waits for the device).</summary>
	public List<Tuple<double, int, double[], Map>> DeviceWayMaps()
	{
		int length; IntPtr times, best, poses, counts, offsets, w, m, c;
		Check(PhdHipLib.phd_map_history(nav, out length, out times, out best, out poses, out counts, out offsets, out w, out m, out c));
		double[] t = new double[length], x = new double[7 * length];
		int[]    b = new int[length], n = new int[length];
		long[]   off = new long[length + 1];
		Marshal.Copy(offsets, off, 0, length + 1);
		if (length > 0) { Marshal.Copy(times, t, 0, length); Marshal.Copy(poses, x, 0, 7 * length); Marshal.Copy(best, b, 0, length); Marshal.Copy(counts, n, 0, length); }
		int      total = (int) off[length];
		double[] ws = new double[total], ms = new double[3 * total], cs = new double[9 * total];
		if (total > 0) { Marshal.Copy(w, ws, 0, total); Marshal.Copy(m, ms, 0, 3 * total); Marshal.Copy(c, cs, 0, 9 * total); }
		var maps = new List<Tuple<double, int, double[], Map>>(length);
		for (int k = 0; k < length; k++) {
			Map map = new Map(3);
			for (long i = off[k]; i < off[k] + n[k]; i++) {
				double[][] cov = { new double[] {cs[9*i], cs[9*i+1], cs[9*i+2]}, new double[] {cs[9*i+3], cs[9*i+4], cs[9*i+5]}, new double[] {cs[9*i+6], cs[9*i+7], cs[9*i+8]} };
				map.Add(new Gaussian(new double[] {ms[3*i], ms[3*i+1], ms[3*i+2]}, cov, ws[i]));
			}
			double[] state = new double[7];
			Array.Copy(x, 7 * k, state, 0, 7);
			maps.Add(Tuple.Create(t[k], b[k], state, map));
		}
		return maps;
	}

	/// <summary>≙ Plot.MapError (postanalysis/Plot.cs:478-529) over the map log, on the device (phd_map_error; waits for it): per
	/// entry (time, OSPA, cardinality part, spatial part, size of Map.BestMapEstimate) against `truth`, the visited map, with
	/// cut-off c and order p. align: null, or per entry the estimated and the true pose at the reference time (14 doubles);
	/// hasreference: null (every entry is aligned) or one byte per entry.</summary>
	public List<Tuple<double, double, double, double, int>> MapError(List<double[]> truth, double c, double p, double[] align, byte[] hasreference)
	{
		double[] t3 = new double[3 * truth.Count];
		for (int i = 0; i < truth.Count; i++) { truth[i].CopyTo(t3, 3 * i); }
		int length; IntPtr times, ospa, card, spatial, sizes;
		fixed (double* pt = t3) fixed (double* pa = align) fixed (byte* ph = hasreference) {
			Check(PhdHipLib.phd_map_error(nav, (IntPtr) pt, truth.Count, c, p, (IntPtr) pa, (IntPtr) ph, out length, out times, out ospa, out card, out spatial, out sizes));
		}
		double[] t = new double[length], o = new double[length], k = new double[length], s = new double[length];
		int[]    n = new int[length];
		if (length > 0) { Marshal.Copy(times, t, 0, length); Marshal.Copy(ospa, o, 0, length); Marshal.Copy(card, k, 0, length); Marshal.Copy(spatial, s, 0, length); Marshal.Copy(sizes, n, 0, length); }
		var series = new List<Tuple<double, double, double, double, int>>(length);
		for (int i = 0; i < length; i++) { series.Add(Tuple.Create(t[i], o[i], k[i], s[i], n[i])); }
		return series;
	}

	/// <summary>≙ Plot.LocationError, RotationError, OdoLocationError and OdoRotationError (postanalysis/Plot.cs:293-456) over the
	/// trajectory log, on the device (phd_pose_error; waits for it), as four TimedValue lists in that order. truth: the true
	/// state at every entry of the log (a TimedState; only the states are read). mode: 0 HistMode.Timed, 1 Smooth, 2 Filter.
	/// slots: null (the best particle of the map log) or per entry the slot whose path is the estimate then. The estimates are
	/// the entries from firstentry on; refentry is Plot.RefTime; slamtime the time of the "SLAM ... on" tag, 0 without one.</summary>
	public List<Tuple<double, double>>[] DevicePoseError(List<Tuple<double, double[]>> truth, int mode, int[] slots, int firstentry, int refentry, double slamtime)
	{
		double[] g7 = new double[7 * truth.Count];
		for (int i = 0; i < truth.Count; i++) { truth[i].Item2.CopyTo(g7, 7 * i); }
		int length, odolength; IntPtr times, loc, rot, odotimes, odoloc, odorot;
		fixed (double* pg = g7) fixed (int* ps = slots) {
			Check(PhdHipLib.phd_pose_error(nav, mode, (IntPtr) pg, truth.Count, (IntPtr) ps, firstentry, refentry, slamtime,
			                               out length, out times, out loc, out rot, out odolength, out odotimes, out odoloc, out odorot));
		}
		return new List<Tuple<double, double>>[] { ToTimedValue(length, times, loc), ToTimedValue(length, times, rot),
		                                           ToTimedValue(odolength, odotimes, odoloc), ToTimedValue(odolength, odotimes, odorot) };
	}

	static List<Tuple<double, double>> ToTimedValue(int length, IntPtr times, IntPtr values)
	{
		double[] t = new double[length], v = new double[length];
		if (length > 0) { Marshal.Copy(times, t, 0, length); Marshal.Copy(values, v, 0, length); }
		var series = new List<Tuple<double, double>>(length);                 // TimedValue
		for (int k = 0; k < length; k++) { series.Add(Tuple.Create(t[k], v[k])); }
		return series;
	}

	/// <summary>≙ static PHDNavigator.QuasiSetLogLikelihood(measurements, map, pose) (PHDNavigator.cs:526-531) for a batch of
	/// candidate poses against one map estimate (the pose searches of LoopyPHDNavigator.cs:777-909).</summary>
	public double[] QuasiSetLogLikelihood(List<PixelRangeMeasurement> measurements, IMap map, Pose3D[] poses)
	{
		double[] z = new double[3 * measurements.Count], lm = new double[3 * map.Count], p7 = new double[7 * poses.Length];
		for (int i = 0; i < measurements.Count; i++) { measurements[i].ToLinear().CopyTo(z, 3 * i); }
		int j = 0;
		foreach (Gaussian landmark in map) { landmark.Mean.CopyTo(lm, 3 * j++); }
		for (int i = 0; i < poses.Length; i++) { poses[i].State.CopyTo(p7, 7 * i); }
		double[] result = new double[poses.Length];
		fixed (double* pz = z) fixed (double* pl = lm) fixed (double* pp = p7) fixed (double* pr = result) {
			Check(PhdHipLib.phd_quasi_set_loglik(nav, (IntPtr) pp, poses.Length, (IntPtr) pl, map.Count, (IntPtr) pz, measurements.Count, (IntPtr) pr));
		}
		return result;
	}

	/// <summary>≙ static PHDNavigator.QuasiSetLogLikelihood(measurements, map, pose, out gradient) (PHDNavigator.cs:543-548)
	/// for a batch of candidate poses: what LogLikeGradientAscent and LogLikeFitCovariance evaluate
	/// (LoopyPHDNavigator.cs:916-1021). averagemode 0 follows TemperedAverage as written, 1 divides its weights by their sum.</summary>
	public double[] QuasiSetLogLikelihood(List<PixelRangeMeasurement> measurements, IMap map, Pose3D[] poses, out double[][] gradients, int averagemode = 0)
	{
		double[] z = new double[3 * measurements.Count], lm = new double[3 * map.Count], p7 = new double[7 * poses.Length];
		for (int i = 0; i < measurements.Count; i++) { measurements[i].ToLinear().CopyTo(z, 3 * i); }
		int j = 0;
		foreach (Gaussian landmark in map) { landmark.Mean.CopyTo(lm, 3 * j++); }
		for (int i = 0; i < poses.Length; i++) { poses[i].State.CopyTo(p7, 7 * i); }
		double[] result = new double[poses.Length], g = new double[6 * poses.Length];
		fixed (double* pz = z) fixed (double* pl = lm) fixed (double* pp = p7) fixed (double* pr = result) fixed (double* pg = g) {
			Check(PhdHipLib.phd_quasi_set_loglik_grad(nav, (IntPtr) pp, poses.Length, (IntPtr) pl, map.Count, (IntPtr) pz, measurements.Count, averagemode, (IntPtr) pr, (IntPtr) pg));
		}
		gradients = new double[poses.Length][];
		for (int i = 0; i < poses.Length; i++) { gradients[i] = new double[6]; Array.Copy(g, 6 * i, gradients[i], 0, 6); }
		return result;
	}

	/// <summary>≙ LoopyPHDNavigator.LogLikeGradientAscent (LoopyPHDNavigator.cs:916-965) for several initial estimates side by
	/// side, resident on the device (phd_quasi_ascent): one call per maxestimates estimates (at most the handle's max_particles / 16).
	/// Returns the maxima as linear poses; loglike[a] is the value at poses[a]. An estimate still climbing after maxiterations
	/// iterations is returned as it stands then and capped is set.</summary>
	public double[][] DeviceLogLikeGradientAscent(double[][] initial, List<PixelRangeMeasurement> measurements, IMap map, Pose3D linearpoint,
	                                              int maxestimates, out double[] loglike, out bool capped, int averagemode = 0, int maxiterations = 1000)
	{
		const int StatusCapacity = 2;                                     // PHD_ERR_CAPACITY
		int n = initial.Length;
		double[] z = new double[3 * measurements.Count], lm = new double[3 * map.Count], p6 = new double[6 * n], lin = linearpoint.State;
		for (int i = 0; i < measurements.Count; i++) { measurements[i].ToLinear().CopyTo(z, 3 * i); }
		int j = 0;
		foreach (Gaussian landmark in map) { landmark.Mean.CopyTo(lm, 3 * j++); }
		for (int i = 0; i < n; i++) { initial[i].CopyTo(p6, 6 * i); }
		double[] result = new double[6 * n];
		int[] iterations = new int[n];
		loglike = new double[n];
		capped = false;
		fixed (double* pz = z) fixed (double* pl = lm) fixed (double* pp = p6) fixed (double* plin = lin) fixed (double* pr = result) fixed (double* pv = loglike) fixed (int* pi = iterations) {
			for (int s = 0; s < n; s += Math.Max(1, maxestimates)) {
				int m = Math.Min(Math.Max(1, maxestimates), n - s);
				int status = PhdHipLib.phd_quasi_ascent(nav, (IntPtr) (pp + 6 * s), m, (IntPtr) plin, (IntPtr) pl, map.Count, (IntPtr) pz, measurements.Count,
				                                        averagemode, maxiterations, 0, (IntPtr) (pr + 6 * s), (IntPtr) (pv + s), (IntPtr) (pi + s), IntPtr.Zero);
				if (status == StatusCapacity) { capped = true; } else { Check(status); }
			}
		}
		double[][] poses = new double[n][];
		for (int i = 0; i < n; i++) { poses[i] = new double[6]; Array.Copy(result, 6 * i, poses[i], 0, 6); }
		return poses;
	}

	/// <summary>DeviceLogLikeGradientAscent for the estimates of many frames in the same launches (phd_quasi_ascent_multi): the
	/// GuidedFitMixture of every frame of UpdateMessagesFromMap (LoopyPHDNavigator.cs:525-551). Frame q has the map estimate
	/// maps[q], the measurements measurements[q] and the linearisation pose linearpoints[q]; estimate a starts at initial[a] and
	/// belongs to frame problem[a]. Every estimate comes back as from DeviceLogLikeGradientAscent with its frame alone. One call
	/// takes frames of one measurement-block class (up to 64, 65 to 128, 129 to 256 measurements; none fits any) and at most the
	/// handle's max_particles / 16 estimates: a caller with more, or with mixed classes, makes several calls.</summary>
	public double[][] DeviceLogLikeGradientAscentMulti(double[][] initial, int[] problem, List<List<PixelRangeMeasurement>> measurements, List<IMap> maps,
	                                                   Pose3D[] linearpoints, out double[] loglike, out bool capped, int averagemode = 0, int maxiterations = 1000)
	{
		const int StatusCapacity = 2;                                     // PHD_ERR_CAPACITY
		int n = initial.Length, np = maps.Count;
		int[] lmoff = new int[np + 1], zoff = new int[np + 1];
		for (int q = 0; q < np; q++) { lmoff[q + 1] = lmoff[q] + maps[q].Count; zoff[q + 1] = zoff[q] + measurements[q].Count; }
		double[] z = new double[3 * zoff[np] + 3], lm = new double[3 * lmoff[np] + 3], p6 = new double[6 * n], lin = new double[7 * np];
		for (int q = 0; q < np; q++) {
			for (int i = 0; i < measurements[q].Count; i++) { measurements[q][i].ToLinear().CopyTo(z, 3 * (zoff[q] + i)); }
			int j = lmoff[q];
			foreach (Gaussian landmark in maps[q]) { landmark.Mean.CopyTo(lm, 3 * j++); }
			linearpoints[q].State.CopyTo(lin, 7 * q);
		}
		for (int i = 0; i < n; i++) { initial[i].CopyTo(p6, 6 * i); }
		double[] result = new double[6 * n];
		int[] iterations = new int[n];
		loglike = new double[n];
		capped = false;
		fixed (double* pz = z) fixed (double* pl = lm) fixed (double* pp = p6) fixed (double* plin = lin) fixed (double* pr = result) fixed (double* pv = loglike)
		fixed (int* pi = iterations) fixed (int* plo = lmoff) fixed (int* pzo = zoff) fixed (int* pq = problem) {
			int status = PhdHipLib.phd_quasi_ascent_multi(nav, np, (IntPtr) plo, (IntPtr) pl, (IntPtr) pzo, (IntPtr) pz, (IntPtr) plin, (IntPtr) pp, (IntPtr) pq, n,
			                                              averagemode, maxiterations, 0, (IntPtr) pr, (IntPtr) pv, (IntPtr) pi, IntPtr.Zero);
			if (status == StatusCapacity) { capped = true; } else { Check(status); }
		}
		double[][] poses = new double[n][];
		for (int i = 0; i < n; i++) { poses[i] = new double[6]; Array.Copy(result, 6 * i, poses[i], 0, 6); }
		return poses;
	}

	/// <summary>The guess loop of GuidedFitMixture (LoopyPHDNavigator.cs:789-797) and the first evaluation of every guess (:808-823)
	/// for many frames in one call (phd_quasi_guesses_multi). Frame q has the map estimate maps[q], the measurements
	/// measurements[q], the linearisation pose linearpoints[q] and the initial linear pose pose0s[q]. guesses[q] is the list the
	/// reference builds: pose0s[q], then, landmark by landmark and measurement by measurement, FitToMeasurement's pose where it lies
	/// within `radius` of the initial pose, as a linear pose around linearpoints[q]; values[q][e] is QuasiSetLogLikelihood at
	/// linearpoints[q].Add(guesses[q][e]) and emptyspace[q] its value at the pose far from everything. The frames of one call lie
	/// in one measurement-block class, as for DeviceLogLikeGradientAscentMulti. A call whose arrays were too small is repeated
	/// once with the total the library reports.</summary>
	public double[][][] DeviceGuidedGuesses(double[][] pose0s, List<List<PixelRangeMeasurement>> measurements, List<IMap> maps, Pose3D[] linearpoints,
	                                        out double[][] values, out double[] emptyspace, double radius = 0.5)
	{
		const int StatusCapacity = 2;                                     // PHD_ERR_CAPACITY
		int np = maps.Count;
		int[] lmoff = new int[np + 1], zoff = new int[np + 1], goff = new int[np + 1];
		for (int q = 0; q < np; q++) { lmoff[q + 1] = lmoff[q] + maps[q].Count; zoff[q + 1] = zoff[q] + measurements[q].Count; }
		double[] z = new double[3 * zoff[np] + 3], lm = new double[3 * lmoff[np] + 3], p6 = new double[6 * np], lin = new double[7 * np];
		for (int q = 0; q < np; q++) {
			for (int i = 0; i < measurements[q].Count; i++) { measurements[q][i].ToLinear().CopyTo(z, 3 * (zoff[q] + i)); }
			int j = lmoff[q];
			foreach (Gaussian landmark in maps[q]) { landmark.Mean.CopyTo(lm, 3 * j++); }
			linearpoints[q].State.CopyTo(lin, 7 * q);
			pose0s[q].CopyTo(p6, 6 * q);
		}
		double[] far = Pose3D.Identity.Add(new double[] {1e5, 1e5, 1e5, 1e5, 1e5, 1e5}).State;   // :808
		emptyspace = new double[np];
		int capacity = np + 64 * np;
		int[] pairs = null;
		double[] g6 = null, p7 = null, v = null;
		for (int attempt = 0; attempt < 2; attempt++) {
			pairs = new int[2 * capacity]; g6 = new double[6 * capacity]; p7 = new double[7 * capacity]; v = new double[capacity];
			int status;
			fixed (double* pz = z) fixed (double* pl = lm) fixed (double* pp = p6) fixed (double* plin = lin) fixed (double* pf = far) fixed (double* pg = g6)
			fixed (double* pq = p7) fixed (double* pv = v) fixed (double* pe = emptyspace) fixed (int* plo = lmoff) fixed (int* pzo = zoff) fixed (int* pgo = goff)
			fixed (int* ppr = pairs) {
				status = PhdHipLib.phd_quasi_guesses_multi(nav, np, (IntPtr) plo, (IntPtr) pl, (IntPtr) pzo, (IntPtr) pz, (IntPtr) plin, (IntPtr) pp, (IntPtr) pf, radius,
				                                           capacity, (IntPtr) pgo, (IntPtr) ppr, (IntPtr) pg, (IntPtr) pq, (IntPtr) pv, (IntPtr) pe);
			}
			if (status == StatusCapacity && attempt == 0) { capacity = goff[np]; continue; }   // (guess_offsets is set: the total)
			Check(status);
			break;
		}
		double[][][] guesses = new double[np][][];
		values = new double[np][];
		for (int q = 0; q < np; q++) {
			int count = goff[q + 1] - goff[q];
			guesses[q] = new double[count][];
			values[q] = new double[count];
			for (int e = 0; e < count; e++) {
				guesses[q][e] = new double[6];
				Array.Copy(g6, 6 * (goff[q] + e), guesses[q][e], 0, 6);
				values[q][e] = v[goff[q] + e];
			}
		}
		return guesses;
	}

	Map MapOfParticle(int particle)
	{
		int n; IntPtr w, m, c;
		Check(PhdHipLib.phd_map(nav, particle, out n, out w, out m, out c));
		double[] ws = new double[n], ms = new double[3 * n], cs = new double[9 * n];
		if (n > 0) { Marshal.Copy(w, ws, 0, n); Marshal.Copy(m, ms, 0, 3 * n); Marshal.Copy(c, cs, 0, 9 * n); }
		Map map = new Map(3);
		for (int i = 0; i < n; i++) {
			double[][] cov = { new double[] {cs[9*i], cs[9*i+1], cs[9*i+2]}, new double[] {cs[9*i+3], cs[9*i+4], cs[9*i+5]}, new double[] {cs[9*i+6], cs[9*i+7], cs[9*i+8]} };
			map.Add(new Gaussian(new double[] {ms[3*i], ms[3*i+1], ms[3*i+2]}, cov, ws[i]));
		}
		return map;
	}

	/// <summary>The maps LoopyPHDNavigator.FilterMissing (LoopyPHDNavigator.cs:729-762) gives for every frame below `to` left out
	/// in turn — the loop of UpdateMessagesFromMap (:511-552) — and Filter's map over those frames (`full`), from one pass over the
	/// frames: the leave-one-out filters are the particles of this handle stepped together, the particle that leaves frame k out
	/// held through step k (phd_step_hold_async); one more particle is never held. This navigator is reset (mapping only, empty
	/// maps); it must have been made for at least to + 1 particles (the Python and C++ mirrors run longer trajectories as several
	/// passes). Nothing waits for the device until the one phd_sync at the end.</summary>
	public Map[] DeviceLeaveOneOutMaps(List<Tuple<double, Pose3D>> trajectory, List<Tuple<double, List<PixelRangeMeasurement>>> factors, int to, out Map full)
	{
		to = Math.Max(0, Math.Min(trajectory.Count, to));
		int count = to + 1;
		double[] pose0 = (trajectory.Count > 0) ? trajectory[0].Item2.State : new double[] {0, 0, 0, 1, 0, 0, 0};
		double[] none = new double[1];
		fixed (double* pp = pose0) fixed (double* pn = none) {
			Check(PhdHipLib.phd_reset(nav, count, (IntPtr) pp, (IntPtr) pn, (IntPtr) pn, (IntPtr) pn, 0));
		}
		double[] poses = new double[7 * count];
		for (int k = 0; k < to; k++) {
			for (int i = 0; i < count; i++) { trajectory[k].Item2.State.CopyTo(poses, 7 * i); }
			List<PixelRangeMeasurement> measurements = factors[k].Item2;
			double[] z = new double[Math.Max(1, 3 * measurements.Count)];
			for (int i = 0; i < measurements.Count; i++) { measurements[i].ToLinear().CopyTo(z, 3 * i); }
			fixed (double* pp = poses) fixed (double* pz = z) {
				Check(PhdHipLib.phd_set_poses(nav, (IntPtr) pp, count));
				Check(PhdHipLib.phd_set_measurements(nav, (IntPtr) pz, measurements.Count));   // (an empty set is a step like any other)
			}
			Check(PhdHipLib.phd_step_hold_async(nav, k));
		}
		Check(PhdHipLib.phd_sync(nav));
		Map[] maps = new Map[to];
		for (int k = 0; k < to; k++) { maps[k] = MapOfParticle(k); }
		full = MapOfParticle(to);
		// the managed mirror of the particle set follows the handle (as reset does)
		VehicleParticles = new TrackVehicle<MeasurerT, Pose3D, PixelRangeMeasurement>[count];
		for (int i = 0; i < count; i++) {
			VehicleParticles[i] = RefVehicle.TrackClone(Config.MotionCovarianceMultiplier, Config.MeasurementCovarianceMultiplier,
			                                            Config.NavigatorPD, Config.NavigatorClutterDensity, true);
		}
		VehicleWeights = new double[count];
		for (int i = 0; i < count; i++) { VehicleWeights[i] = 1.0 / count; }
		BestParticle = 0;
		return maps;
	}

	/// <summary>≙ PHDNavigator.SlamUpdate (PHDNavigator.cs:323-362).</summary>
	public override void SlamUpdate(GameTime time, List<PixelRangeMeasurement> measurements)
	{
		double[] z = new double[3 * measurements.Count];
		for (int i = 0; i < measurements.Count; i++) { measurements[i].ToLinear().CopyTo(z, 3 * i); }
		double u = (double) Util.Uniform.Next();                           // PHDNavigator.cs:727: the RNG stays managed
		BeforeSlamUpdate();
		fixed (double* pz = z) { Check(PhdHipLib.phd_slam_update(nav, (IntPtr) pz, measurements.Count, OnlyMapping, u)); }

		int n; bool resampled;
		Marshal.Copy(PhdHipLib.phd_weights(nav, out n), VehicleWeights, 0, VehicleWeights.Length);
		BestParticle = PhdHipLib.phd_best_particle(nav);
		IntPtr src = PhdHipLib.phd_resample_sources(nav, out n, out resampled);
		if (resampled) {                                                    // apply the device's choice to the managed particles
			int[] sources = new int[n];
			Marshal.Copy(src, sources, 0, n);
			var particles = new TrackVehicle<MeasurerT, Pose3D, PixelRangeMeasurement>[n];
			for (int i = 0; i < n; i++) { particles[i] = RefVehicle.TrackClone(VehicleParticles[sources[i]], true); }   // :740
			VehicleParticles = particles;
		}
		UpdateMapHistory(time);
		if (DeviceMapHistory) { AppendDeviceMapHistory(time); }
	}

	protected override void StartSlamInternal()    { Collapse(ParticleCount); }
	protected override void StartMappingInternal() { Collapse(1); }

	void Collapse(int particlecount)                                       // CollapseParticles, PHDNavigator.cs:233-236
	{
		Map best = BestMapModel;
		List<Gaussian> l = best.ToList();
		double[] w = new double[l.Count], m = new double[3 * l.Count], c = new double[9 * l.Count];
		for (int i = 0; i < l.Count; i++) {
			w[i] = l[i].Weight; l[i].Mean.CopyTo(m, 3 * i);
			for (int k = 0; k < 9; k++) { c[9 * i + k] = l[i].Covariance[k / 3][k % 3]; }
		}
		reset(RefVehicle, w, m, c, particlecount);
	}

	public override void Dispose() { if (nav.Handle != IntPtr.Zero) { PhdHipLib.phd_destroy(nav); nav = new HandleRef(this, IntPtr.Zero); } }
}

/// <summary>The PRM3D solver (Program.cs `-i` simulation / record inputs).</summary>
public class HipPHDNavigator : HipPHDNavigatorCore<PRM3DMeasurer>
{
	public HipPHDNavigator(Vehicle<PRM3DMeasurer, Pose3D, PixelRangeMeasurement> vehicle, int particlecount, bool onlymapping = false, int gpus = 1)
		: base(vehicle, particlecount, onlymapping, gpus) { }
}

/// <summary>
/// The Kinect solver (Program.cs:197-204, `-i kinect`): the same body with KinectMeasurer's occlusion-aware detection
/// probability (KinectMeasurer.cs:151-173), fed with the current depth frame before every step (phd_set_depth_map).
/// Wiring: in Simulation.FromFiles, for VehicleType.Kinect with MeasurerT == KinectMeasurer, construct this class where the
/// switch of Simulation.cs:352-379 constructs the navigator.
/// </summary>
public unsafe class HipKinectPHDNavigator : HipPHDNavigatorCore<KinectMeasurer>
{
	float[] frame = new float[0];

	public HipKinectPHDNavigator(Vehicle<KinectMeasurer, Pose3D, PixelRangeMeasurement> vehicle, int particlecount, bool onlymapping = false, int gpus = 1)
		: base(vehicle, particlecount, onlymapping, gpus) { }

	/// <summary>KinectTrackVehicle (KinectTrackVehicle.cs:66-68): the particles' film is the explorer's inflated by -Border.</summary>
	protected override void AdjustParams(ref PhdParams p, Vehicle<KinectMeasurer, Pose3D, PixelRangeMeasurement> vehicle)
	{
		int border = ((KinectVehicle) vehicle).Border;
		p.measurer[3] += border; p.measurer[4] += border;           // Rectangle.Inflate(-Border, -Border)
		p.measurer[5] -= 2 * border; p.measurer[6] -= 2 * border;
	}

	/// <summary>The particles' GetDepth() closure returns the current frame, float[ResX][ResY] indexed [x][y]; the library takes
	/// it row-major, depth[y * ResX + x]. Values go as they are (no unit conversion: INTEGRATION.md, "Kinect input").</summary>
	protected override void BeforeSlamUpdate()
	{
		float[][] depth = VehicleParticles[0].Measurer.GetDepth();
		int w = depth.Length, h = (w > 0) ? depth[0].Length : 0;
		if (w == 0 || h == 0) { Check(PhdHipLib.phd_set_depth_map(nav, IntPtr.Zero, 0, 0)); return; }
		if (frame.Length != w * h) { frame = new float[w * h]; }
		for (int x = 0; x < w; x++) {
			float[] column = depth[x];
			for (int y = 0; y < h; y++) { frame[y * w + x] = column[y]; }
		}
		fixed (float* pf = frame) { Check(PhdHipLib.phd_set_depth_map(nav, (IntPtr) pf, w, h)); }
	}
}
}
