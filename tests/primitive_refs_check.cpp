// primitive_refs_check.cpp — host transcriptions of the device primitives whose bounds tests/primitive_cases.py derives:
// exp_neg, exp_pair, gauss_logw, the double-double helpers, slot_target and small_div, written again from their statement in
// monorfs_amd/csrc/phd_device.h and phd_resample.h in exactly rounded host arithmetic (std::fma is the correctly rounded
// fused multiply-add; built with -ffp-contract=off, so nothing else fuses). tests/test_primitive_refs.py runs the generators
// and the assertions of the device test through it: the references stay inside their own bounds before a GPU is asked.
//
//   primitive_refs_check OP in.bin out.bin table.bin
// The record layouts are those of phd_primitives_test.h; table.bin: 256 doubles, 2^(j/256) correctly rounded.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static double T[256];

static double exp_neg(double x)
{
	x = (x < -800.0) ? -800.0 : x;
	const double n = std::rint(x * 369.3299304675746);
	double r = std::fma(-n, 0.002707606166950427, x);
	r = std::fma(-n, 7.111859369156821e-12, r);
	const int ni = std::isnan(n) ? 0 : (int) n;      // (the device's conversion of a NaN gives 0)
	const double t = T[ni & 255];
	double p = std::fma(r, 0.041666666666666664, 0.16666666666666666);
	p = std::fma(p, r, 0.5);
	p = std::fma(p, r, 1.0);
	p = std::fma(p, r, 1.0);
	return std::ldexp(t * p, ni >> 8);
}

static double exp_pair(double x, bool keep)
{
	x = (x > -800.0) ? x : -800.0;                    // v_max_f64 x, -800: a NaN gives the other operand
	const double nd = std::fma(x, 369.3299304675746, 6755399441055744.0);
	int64_t b;
	std::memcpy(&b, &nd, 8);
	const int ni = (int) (uint32_t) b;                // the low word of the sum
	const double n = nd - 6755399441055744.0;
	const double r = std::fma(-n, 0.0027076061740622863, x);
	const double t = T[ni & 255];
	double p = std::fma(0.16666666666666666, r, 0.5);
	p = std::fma(p, r, 1.0);
	p = std::fma(p, r, 1.0);
	return std::ldexp(t * p, keep ? (ni >> 8) : -4096);
}

static double gauss_logw(const double* g, double d0, double d1, double d2)
{
	const double t0 = std::fma(g[5], d2, std::fma(g[4], d1, g[3] * d0));
	const double t1 = std::fma(g[7], d2, g[6] * d1);
	const double t2 = g[8] * d2;
	return std::fma(t0, d0, std::fma(t1, d1, std::fma(t2, d2, g[9])));
}

struct dd { double hi, lo; };

static dd two_sum(double a, double b)
{
	double s = a + b, bb = s - a;
	double e = (a - (s - bb)) + (b - bb);
	return dd{s, e};
}

static dd quick(double a, double b)
{
	double s = a + b;
	return dd{s, b - (s - a)};
}

static dd dd_add(dd x, dd y)
{
	dd s = two_sum(x.hi, y.hi);
	dd t = two_sum(x.lo, y.lo);
	s.lo += t.hi;
	s = quick(s.hi, s.lo);
	s.lo += t.lo;
	return quick(s.hi, s.lo);
}

static dd dd_add_d(dd x, double d)
{
	dd s = two_sum(x.hi, d);
	s.lo += x.lo;
	return quick(s.hi, s.lo);
}

static dd slot_target(int i, double R0, double invP)
{
	const double ph = (double) i * invP, pl = std::fma((double) i, invP, -ph);
	return dd_add_d(dd{ph, pl}, R0);
}

// the shuffles of dd_wave_scan on a wave held in an array: every level reads the values of the level before
static void wave_scan(dd* v, int width)
{
	for (int o = 1; o < width; o <<= 1) {
		dd w[64];
		for (int l = 0; l < 64; l++) w[l] = (l >= o) ? dd_add(v[l - o], v[l]) : v[l];
		std::memcpy(v, w, sizeof w);
	}
}

static int small_div(int s, int d, float rd)
{
	int q = (int) ((float) s * rd);
	q -= (q * d > s) ? 1 : 0;
	q += ((q + 1) * d <= s) ? 1 : 0;
	return q;
}

static std::vector<char> slurp(const char* path)
{
	std::vector<char> v;
	FILE* f = std::fopen(path, "rb");
	if (!f) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(2); }
	char buf[1 << 16];
	size_t k;
	while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
	std::fclose(f);
	return v;
}

int main(int argc, char** argv)
{
	if (argc != 5) { std::fprintf(stderr, "usage: primitive_refs_check OP in out table\n"); return 2; }
	const std::string op = argv[1];
	const std::vector<char> in = slurp(argv[2]), tab = slurp(argv[4]);
	if (tab.size() != sizeof T) { std::fprintf(stderr, "the table holds %zu bytes\n", tab.size()); return 2; }
	std::memcpy(T, tab.data(), sizeof T);
	const double* f = (const double*) in.data();
	const uint64_t* u = (const uint64_t*) in.data();
	std::vector<double> out;
	std::vector<uint64_t> outu;
	auto put = [&](dd r) { out.push_back(r.hi); out.push_back(r.lo); };
	auto records = [&](size_t bytes) {
		if (in.size() % bytes) { std::fprintf(stderr, "%s: %zu bytes are no whole records of %zu\n", op.c_str(), in.size(), bytes); std::exit(2); }
		return in.size() / bytes;
	};
	if (op == "PT_EXP_NEG") {
		for (size_t i = 0, n = records(8); i < n; i++) out.push_back(exp_neg(f[i]));
	} else if (op == "PT_EXP_TAB") {
		out.assign(T, T + 256);
	} else if (op == "PT_EXP_PAIR") {
		for (size_t i = 0, n = records(16); i < n; i++) out.push_back(exp_pair(f[2 * i], u[2 * i + 1] != 0));
	} else if (op == "PT_GAUSS_LOGW") {
		for (size_t i = 0, n = records(104); i < n; i++) {
			const double* g = f + 13 * i;
			const double l = gauss_logw(g, g[10] - g[0], g[11] - g[1], g[12] - g[2]);
			out.push_back(l);
			out.push_back(exp_pair(l, true));
		}
	} else if (op == "PT_DD_TWO_SUM") {
		for (size_t i = 0, n = records(16); i < n; i++) put(two_sum(f[2 * i], f[2 * i + 1]));
	} else if (op == "PT_DD_QUICK") {
		for (size_t i = 0, n = records(16); i < n; i++) put(quick(f[2 * i], f[2 * i + 1]));
	} else if (op == "PT_DD_TWO_SUM_PROD") {
		for (size_t i = 0, n = records(24); i < n; i++) put(two_sum(f[3 * i] * f[3 * i + 1], f[3 * i + 2]));
	} else if (op == "PT_DD_ADD") {
		for (size_t i = 0, n = records(32); i < n; i++) put(dd_add(dd{f[4 * i], f[4 * i + 1]}, dd{f[4 * i + 2], f[4 * i + 3]}));
	} else if (op == "PT_DD_ADD_D") {
		for (size_t i = 0, n = records(24); i < n; i++) put(dd_add_d(dd{f[3 * i], f[3 * i + 1]}, f[3 * i + 2]));
	} else if (op == "PT_DD_SCAN_64" || op == "PT_DD_SCAN_16") {
		for (size_t w = 0, n = records(16 * 64); w < n; w++) {
			dd v[64];
			for (int l = 0; l < 64; l++) v[l] = dd{f[2 * (64 * w + l)], f[2 * (64 * w + l) + 1]};
			wave_scan(v, op == "PT_DD_SCAN_64" ? 64 : 16);
			for (int l = 0; l < 64; l++) put(v[l]);
		}
	} else if (op == "PT_SLOT_TARGET") {
		for (size_t i = 0, n = records(24); i < n; i++) put(slot_target((int) (int64_t) u[3 * i], f[3 * i + 1], f[3 * i + 2]));
	} else if (op == "PT_SMALL_DIV") {
		const int32_t* d = (const int32_t*) in.data();
		for (size_t i = 0, n = records(4); i < n; i++) {
			const float rd = 1.0f / (float) d[i];
			uint64_t bad = 0, first = 0;
			for (int s = (1 << 24) - 1; s >= 0; s--) {
				if (small_div(s, d[i], rd) != s / d[i]) { bad++; first = (uint64_t) ((1 << 24) - s); }
			}
			outu.push_back(bad);
			outu.push_back(first);
		}
	} else {
		std::fprintf(stderr, "no transcription of %s\n", op.c_str());
		return 3;
	}
	FILE* o = std::fopen(argv[3], "wb");
	if (!o) return 2;
	if (!out.empty()) std::fwrite(out.data(), 8, out.size(), o);
	if (!outu.empty()) std::fwrite(outu.data(), 8, outu.size(), o);
	std::fclose(o);
	return 0;
}
