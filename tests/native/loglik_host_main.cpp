// Stand-alone driver of the log-likelihood's host code (ctcdecode_amd/csrc/loglik.h through tests/native/loglik_host.cpp), meant to be
// built with -fsanitize=address,undefined.  Every argument is a case file tests/test_loglik_host.py wrote -- the inputs and the outputs
// the Python restatement expects -- and the twin's outputs are compared with them bit for bit; then rows made here: out-of-range labels
// and lengths, lse3 against this box's libm on random and special triples, and random rows against a float64 recurrence.  Every buffer is
// sized exactly, so that an index that escapes its check is a sanitizer report.  Prints "<checks> checks, <n> failures".
//
// Case file: int32 {B, T, V, R, L_stride, blank, log_input, dtype, has_seq_lens}, then rows (B*T*V elements of 4 or 2 bytes), seq_lens
// (B, if any), tokens (B*R*L_stride), lens (B*R), and the expectation: loglik (B*R floats), status (B).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "loglik_host.cpp"

namespace {

long long checks = 0, failures = 0;
void expect(bool ok, const char *what, long long a = 0, long long b = 0) {
  ++checks;
  if (!ok) { ++failures; std::printf("FAIL %s (%lld, %lld)\n", what, a, b); }
}

struct Rng {
  unsigned long long s;
  unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); }
  int below(int n) { return n > 0 ? (int)(next() % (unsigned)n) : 0; }
};

template <typename T> bool read_vec(std::FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

void run_file(const char *path) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f) { expect(false, "case file opens"); return; }
  int32_t h[9];
  if (std::fread(h, 4, 9, f) != 9) { expect(false, "case header"); std::fclose(f); return; }
  const int B = h[0], T = h[1], V = h[2], R = h[3], Ls = h[4], blank = h[5], log_input = h[6], dtype = h[7];
  const size_t eb = dtype == 0 ? 4 : 2, n_rows = (size_t)B * T * V, n_tok = (size_t)B * R * Ls, n_hyp = (size_t)B * R;
  std::vector<unsigned char> rows;
  std::vector<int32_t> seq, tok, lens, want_status;
  std::vector<float> want;
  bool ok = read_vec(f, rows, n_rows * eb) && read_vec(f, seq, h[8] ? (size_t)B : 0) && read_vec(f, tok, n_tok) && read_vec(f, lens, n_hyp) &&
            read_vec(f, want, n_hyp) && read_vec(f, want_status, (size_t)B);
  std::fclose(f);
  if (!ok) { expect(false, "case body"); return; }
  std::vector<int32_t> status((size_t)B, 0);
  std::vector<float> out(n_hyp, -123.0f);
  const int rc = ctcloglik_host_loglik(rows.data(), dtype, h[8] ? seq.data() : nullptr, B, T, V, blank, log_input, tok.data(), lens.data(), R, Ls, out.data(), status.data());
  expect(rc >= 0, "the twin takes the case", rc);
  expect(std::memcmp(out.data(), want.data(), n_hyp * 4) == 0, "loglik == the restatement's, bit for bit");
  expect(std::memcmp(status.data(), want_status.data(), (size_t)B * 4) == 0, "status == the restatement's");
}

// lse3 against the definition evaluated with this box's libm
float lse3_libm(float v0, float v1, float v2) {
  const float m = std::fmax(std::fmax(v0, v1), v2);
  if (m == -INFINITY) return -INFINITY;
  volatile float e0 = expf(v0 - m), e1 = expf(v1 - m), e2 = expf(v2 - m);
  volatile float s01 = e0 + e1;
  volatile float s = s01 + e2;
  volatile float l = logf(s);
  return l + m;
}
void run_lse3(Rng &r) {
  const float special[] = {-INFINITY, -0.0f, 0.0f, -1.0f, -88.0f, -88.5f, -87.5f, -89.0f, -103.9f, -104.5f, -200.0f, -3.0e38f, 5.0f, -1.0e-30f};
  const int ns = (int)(sizeof(special) / sizeof(special[0]));
  long long bad = 0;
  for (int i = 0; i < ns; ++i)
    for (int j = 0; j < ns; ++j)
      for (int k = 0; k < ns; ++k) {
        const float got = ctcloglik_host_lse3(special[i], special[j], special[k]), want = lse3_libm(special[i], special[j], special[k]);
        bad += std::memcmp(&got, &want, 4) != 0;
      }
  expect(bad == 0, "lse3 == the libm formula on the special triples", bad);
  bad = 0;
  for (int i = 0; i < 200000; ++i) {
    float v[3];
    for (float &x : v) {
      const int kind = r.below(8);
      x = kind == 0 ? -INFINITY : -(float)r.below(1 << 20) / (float)(1 << (4 + r.below(14)));
      if (kind == 1) x = -x;
    }
    const float got = ctcloglik_host_lse3(v[0], v[1], v[2]), want = lse3_libm(v[0], v[1], v[2]);
    bad += std::memcmp(&got, &want, 4) != 0;
  }
  expect(bad == 0, "lse3 == the libm formula on random triples", bad);
}

// one item of random log-probabilities and random rows against a float64 recurrence: within n * 2^-23 * (A + 3)
void run_random(Rng &r, int T, int V, int R, int Ls, int blank, bool with_inf) {
  std::vector<float> lp((size_t)T * V);
  for (auto &v : lp) v = -0.125f * (float)r.below(64);
  if (with_inf && T > 2)
    for (int c = 0; c < V; ++c)
      if (c != blank && r.below(3) == 0) lp[(size_t)(T / 2) * V + c] = -INFINITY;
  std::vector<int32_t> tok((size_t)R * Ls, 0), lens((size_t)R, 0), status(1, 0);
  std::vector<float> out((size_t)R, -123.0f);
  for (int p = 0; p < R; ++p) {
    const int L = r.below(Ls + 1);
    lens[(size_t)p] = L;
    for (int i = 0; i < L; ++i) {
      int c = r.below(V - 1);
      if (c >= blank) ++c;
      tok[(size_t)p * Ls + i] = (i > 0 && r.below(4) == 0) ? tok[(size_t)p * Ls + i - 1] : c;
    }
  }
  const int32_t n_arr[1] = {T - r.below(2)};
  const int n = n_arr[0] < 0 ? 0 : n_arr[0];
  const int rc = ctcloglik_host_loglik(lp.data(), 0, n_arr, 1, T, V, blank, 1, tok.data(), lens.data(), R, Ls, out.data(), status.data());
  expect(rc == 0 && status[0] == 0, "valid rows raise nothing", rc, status[0]);
  for (int p = 0; p < R; ++p) {
    const int L = lens[(size_t)p], S = 2 * L + 1;
    const int32_t *y = tok.data() + (size_t)p * Ls;
    if (n == 0 || L > n) {
      expect(out[(size_t)p] == (n == 0 && L == 0 ? 0.0f : -INFINITY), "a row without frames or without room", p);
      continue;
    }
    auto lae = [](double x, double z) {
      const double m = x > z ? x : z;
      return m == -INFINITY ? m : m + std::log(std::exp(x - m) + std::exp(z - m));
    };
    std::vector<double> a((size_t)S, -INFINITY), na((size_t)S);
    double big = 0.0;
    for (int s = 0; s < S && s < 2; ++s) a[(size_t)s] = lp[(size_t)((s & 1) ? y[0] : blank)];
    for (int t = 1; t < n; ++t) {
      for (int s = 0; s < S; ++s) {
        double v = a[(size_t)s];
        if (s >= 1) v = lae(v, a[(size_t)s - 1]);
        if ((s & 1) && s >= 3 && y[s >> 1] != y[(s >> 1) - 1]) v = lae(v, a[(size_t)s - 2]);
        na[(size_t)s] = (double)lp[(size_t)t * V + ((s & 1) ? y[s >> 1] : blank)] + v;
        if (std::isfinite(na[(size_t)s]) && std::fabs(na[(size_t)s]) > big) big = std::fabs(na[(size_t)s]);
      }
      a.swap(na);
    }
    const double ll = L >= 1 ? lae(a[(size_t)S - 1], a[(size_t)S - 2]) : a[(size_t)S - 1];
    if (!std::isfinite(ll)) expect(out[(size_t)p] == -INFINITY, "a row no alignment fits is -inf", p);
    else expect(std::fabs((double)out[(size_t)p] - ll) <= (double)n * std::ldexp(1.0, -23) * (big + 3.0), "within the float32 bound of the float64 recurrence", p);
  }
}

// rows with out-of-range labels and lengths between valid ones: output 0, the status raised, the valid rows untouched by it
void run_invalid(Rng &r) {
  const int T = 12, V = 5, R = 6, Ls = 7, blank = 1;
  std::vector<float> lp((size_t)2 * T * V);
  for (auto &v : lp) v = -0.25f * (float)(1 + r.below(16));
  std::vector<int32_t> tok((size_t)2 * R * Ls, 2), lens((size_t)2 * R, 3);
  auto row = [&](int b, int p) { return &tok[((size_t)b * R + p) * Ls]; };
  row(0, 1)[1] = V;            // a label = V
  row(0, 2)[0] = blank;        // a label = blank
  row(0, 3)[2] = -1;           // a negative label
  lens[4] = -1;                // a negative length
  lens[5] = Ls + 1;            // a length beyond the stride
  row(0, 0)[5] = 1 << 30;      // (beyond the row's length: never looked at)
  std::vector<int32_t> status(2, 0);
  std::vector<float> out((size_t)2 * R, -123.0f);
  const int rc = ctcloglik_host_loglik(lp.data(), 0, nullptr, 2, T, V, blank, 1, tok.data(), lens.data(), R, Ls, out.data(), status.data());
  expect(rc == 5, "five invalid rows", rc);
  expect(status[0] == ctcalign::ALIGN_BAD_ROW && status[1] == 0, "the status of the item with invalid rows alone", status[0], status[1]);
  for (int p = 1; p < R; ++p) expect(out[(size_t)p] == 0.0f, "an invalid row's output is 0", p);
  expect(std::isfinite(out[0]) && out[0] < 0.0f && std::isfinite(out[(size_t)R]), "the valid rows are scored");
}

}  // namespace

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) run_file(argv[i]);
  Rng r{20261020ull};
  run_invalid(r);
  run_lse3(r);
  const int Ts[] = {1, 2, 3, 15, 16, 17, 40};
  for (int T : Ts)
    for (int rep = 0; rep < 6; ++rep) run_random(r, T, 2 + r.below(5), 5, T + (rep % 3) - 1 < 0 ? 0 : T + (rep % 3) - 1, 0, rep >= 4);
  for (int rep = 0; rep < 4; ++rep) run_random(r, 150, 4, 3, 140, 2, false);  // (S beyond 256)
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
