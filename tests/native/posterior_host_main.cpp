// Stand-alone driver of the label posteriors' host code (ctcdecode_amd/csrc/posterior.h through tests/native/posterior_host.cpp), meant
// to be built with -fsanitize=address,undefined.  Every argument is a case file tests/test_posterior_host.py wrote -- the inputs and the
// outputs the Python restatement expects -- and the twin's outputs are compared with them bit for bit; then rows made here:
// out-of-range labels and lengths, e80 against this box's libm, and random rows against the properties the definition implies.  Every
// buffer is sized exactly (the scratch slot by the twin itself), so that an index that escapes its check is a sanitizer report.
// Prints "<checks> checks, <n> failures".
//
// Case file: int32 {B, T, V, R, L_stride, blank, log_input, dtype, has_seq_lens}, then rows (B*T*V elements of 4 or 2 bytes), seq_lens
// (B, if any), tokens (B*R*L_stride), lens (B*R), and the expectation: peaks (B*R*L_stride int32), occupancy, confidence (B*R*L_stride
// floats each), loglik (B*R floats), status (B).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "posterior_host.cpp"

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

struct Outputs {
  std::vector<int32_t> peaks, status;
  std::vector<float> occ, conf, ll;
  Outputs(size_t B, size_t hyps, size_t labels) : peaks(labels, 0x5A5A5A5A), status(B, 0), occ(labels, -123.0f), conf(labels, -123.0f), ll(hyps, -123.0f) {}
};

void run_file(const char *path) {
  std::FILE *f = std::fopen(path, "rb");
  if (!f) { expect(false, "case file opens"); return; }
  int32_t h[9];
  if (std::fread(h, 4, 9, f) != 9) { expect(false, "case header"); std::fclose(f); return; }
  const int B = h[0], T = h[1], V = h[2], R = h[3], Ls = h[4], blank = h[5], log_input = h[6], dtype = h[7];
  const size_t eb = dtype == 0 ? 4 : 2, n_rows = (size_t)B * T * V, n_tok = (size_t)B * R * Ls, n_hyp = (size_t)B * R;
  std::vector<unsigned char> rows;
  std::vector<int32_t> seq, tok, lens, want_peaks, want_status;
  std::vector<float> want_occ, want_conf, want_ll;
  bool ok = read_vec(f, rows, n_rows * eb) && read_vec(f, seq, h[8] ? (size_t)B : 0) && read_vec(f, tok, n_tok) && read_vec(f, lens, n_hyp) &&
            read_vec(f, want_peaks, n_tok) && read_vec(f, want_occ, n_tok) && read_vec(f, want_conf, n_tok) && read_vec(f, want_ll, n_hyp) &&
            read_vec(f, want_status, (size_t)B);
  std::fclose(f);
  if (!ok) { expect(false, "case body"); return; }
  Outputs o((size_t)B, n_hyp, n_tok);
  const int rc = ctcpost_host_posteriors(rows.data(), dtype, h[8] ? seq.data() : nullptr, B, T, V, blank, log_input, tok.data(), lens.data(), R, Ls, o.peaks.data(),
                                         o.occ.data(), o.conf.data(), o.ll.data(), o.status.data());
  expect(rc >= 0, "the twin takes the case", rc);
  expect(std::memcmp(o.peaks.data(), want_peaks.data(), n_tok * 4) == 0, "peaks == the restatement's");
  expect(std::memcmp(o.occ.data(), want_occ.data(), n_tok * 4) == 0, "occupancy == the restatement's, bit for bit");
  expect(std::memcmp(o.conf.data(), want_conf.data(), n_tok * 4) == 0, "confidence == the restatement's, bit for bit");
  expect(std::memcmp(o.ll.data(), want_ll.data(), n_hyp * 4) == 0, "loglik == the restatement's, bit for bit");
  expect(std::memcmp(o.status.data(), want_status.data(), (size_t)B * 4) == 0, "status == the restatement's");
}

// e80 against the definition evaluated with this box's libm
void run_e80(Rng &r) {
  const float special[] = {-INFINITY, -0.0f, 0.0f, 1.0e-7f, 3.0f, -80.0f, -80.00001f, -79.99999f, -1.0f, -87.0f, -3.0e38f, -1.0e-30f, -40.0f, -55.0f};
  long long bad = 0;
  auto want = [](float x) {
    if (x > 0.0f) x = 0.0f;
    if (x < -80.0f) return 0.0f;
    return expf(x);
  };
  for (float x : special) {
    const float got = ctcpost_host_e80(x), w = want(x);
    bad += std::memcmp(&got, &w, 4) != 0;
  }
  for (int i = 0; i < 200000; ++i) {
    const float x = 1.0f - (float)r.below(1 << 20) / (float)(1 << (6 + r.below(12)));
    const float got = ctcpost_host_e80(x), w = want(x);
    bad += std::memcmp(&got, &w, 4) != 0;
  }
  expect(bad == 0, "e80 == the libm formula", bad);
  expect(ctcpost_host_g(-INFINITY, -1.0f, -1.0f, -2.0f) == 0.0f && ctcpost_host_g(-1.0f, -INFINITY, -1.0f, -2.0f) == 0.0f, "g is 0 without a or b");
  expect(ctcpost_host_g(-3.0e38f, -3.0e38f, -1.0f, -2.0f) == 0.0f, "g is 0 where a + b overflows");
  expect(ctcpost_host_g(-INFINITY, -INFINITY, -INFINITY, -2.0f) == 0.0f, "g is 0 for an impossible label");
  expect(ctcpost_host_g(-3.0f, -4.0f, -1.0f, -6.0f) == 1.0f && ctcpost_host_g(-3.0f, -4.0f, -1.0f, -6.5f) == 1.0f, "g of an exact or an exceeded ll is 1");
}

// one item of random log-probabilities and random rows: what the definition implies for every valid row with alignments --
// peaks in [0, n), occupancy in [0, n], confidence in [0, 1], the occupancies of a row's labels sum to at most n and each is at least
// 1 (a label occupies a frame on every alignment), all within the 5 % that n <= 150 frames of float32 sums near -1000 can move a
// posterior (n x 3 x 2^-13 in the exponent) -- and zero tails
void run_random(Rng &r, int T, int V, int R, int Ls, int blank, bool with_inf) {
  std::vector<float> lp((size_t)T * V);
  for (auto &v : lp) v = -0.125f * (float)r.below(64);
  if (with_inf && T > 2)
    for (int c = 0; c < V; ++c)
      if (c != blank && r.below(3) == 0) lp[(size_t)(T / 2) * V + c] = -INFINITY;
  std::vector<int32_t> tok((size_t)R * Ls, 0), lens((size_t)R, 0);
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
  Outputs o(1, (size_t)R, (size_t)R * Ls);
  const int rc = ctcpost_host_posteriors(lp.data(), 0, n_arr, 1, T, V, blank, 1, tok.data(), lens.data(), R, Ls, o.peaks.data(), o.occ.data(), o.conf.data(), o.ll.data(),
                                         o.status.data());
  expect(rc == 0 && o.status[0] == 0, "valid rows raise nothing", rc, o.status[0]);
  for (int p = 0; p < R; ++p) {
    const int L = lens[(size_t)p];
    const size_t at = (size_t)p * Ls;
    const bool runs = n >= 1 && L <= n && o.ll[(size_t)p] > -INFINITY;
    bool ok = true;
    double sum = 0.0;
    for (int i = 0; i < Ls; ++i) {
      const float oc = o.occ[at + i], cf = o.conf[at + i];
      const int pk = o.peaks[at + i];
      if (i >= L || !runs) ok = ok && pk == 0 && oc == 0.0f && cf == 0.0f;
      else {
        ok = ok && pk >= 0 && pk < n && oc >= 0.9f && oc <= (float)n * 1.05f && cf >= 0.0f && cf <= 1.0f;
        sum += oc;
      }
    }
    expect(ok, "a row's outputs are in range and its tails are 0", p, L);
    expect(sum <= (double)n * 1.05, "the labels of a row occupy at most the item's frames", p);
  }
}

// rows with out-of-range labels and lengths between valid ones: outputs 0, the status raised, the valid rows untouched by it
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
  Outputs o(2, (size_t)2 * R, (size_t)2 * R * Ls);
  const int rc = ctcpost_host_posteriors(lp.data(), 0, nullptr, 2, T, V, blank, 1, tok.data(), lens.data(), R, Ls, o.peaks.data(), o.occ.data(), o.conf.data(), o.ll.data(),
                                         o.status.data());
  expect(rc == 5, "five invalid rows", rc);
  expect(o.status[0] == ctcalign::ALIGN_BAD_ROW && o.status[1] == 0, "the status of the item with invalid rows alone", o.status[0], o.status[1]);
  for (int p = 1; p < R; ++p) {
    bool zero = o.ll[(size_t)p] == 0.0f;
    for (int i = 0; i < Ls; ++i) zero = zero && o.peaks[(size_t)p * Ls + i] == 0 && o.occ[(size_t)p * Ls + i] == 0.0f && o.conf[(size_t)p * Ls + i] == 0.0f;
    expect(zero, "an invalid row's outputs are 0", p);
  }
  expect(std::isfinite(o.ll[0]) && o.ll[0] < 0.0f && o.occ[0] >= 0.9f && std::isfinite(o.ll[(size_t)R]), "the valid rows are scored");
}

}  // namespace

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) run_file(argv[i]);
  Rng r{20261020ull};
  run_invalid(r);
  run_e80(r);
  const int Ts[] = {1, 2, 3, 15, 16, 17, 40};
  for (int T : Ts)
    for (int rep = 0; rep < 6; ++rep) run_random(r, T, 2 + r.below(5), 5, T + (rep % 3) - 1 < 0 ? 0 : T + (rep % 3) - 1, 0, rep >= 4);
  for (int rep = 0; rep < 4; ++rep) run_random(r, 150, 4, 3, 140, 2, false);  // (S beyond 256: the slot's long-row share)
  std::printf("%lld checks, %lld failures\n", checks, failures);
  return failures ? 1 : 0;
}
