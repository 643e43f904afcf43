// Host twin of the stream images (ctcdecode_amd/csrc/stream_snapshot.h): the stream of commit_host.cpp -- the host build of the core
// fed chunk by chunk, peek, compaction and commit run on its parked state, the product's capacity bookkeeping -- saved to an image
// and restored from one with the same routines the kernels of stream_snapshot.hip run, under a sequential policy.  Test
// infrastructure only.  (commit_host.cpp, and compact_host.cpp / peek_host.cpp / core_host.cpp through it, are compiled into this
// library as they are.)
#include "commit_host.cpp"

#include "../../ctcdecode_amd/csrc/stream_snapshot.h"

namespace {

ctcsnap::SnapExpect expect_of(const PeekStream &s) {
  ctcsnap::SnapExpect e;
  e.K = s.beam; e.V = s.V;
  e.scorer_kind = s.lm ? ctcsnap::SNAP_SCORER_BUILTIN : ctcsnap::SNAP_SCORER_NONE;
  e.fingerprint = s.lm ? ctcsnap::scorer_fingerprint(s.hs) : 0ull;
  e.lm_states = s.lm ? (long long)s.hs.st_bo.size() : 0;
  e.lm_dict = s.lm ? (long long)s.hs.dict.size() : 0;
  e.lm_dict_lab = s.lm ? (long long)s.hs.dict_lab.size() : 0;
  e.lm_char_based = s.lm && s.hs.char_based ? 1 : 0;
  e.lm_dict_wide = s.lm ? s.view.dict_wide : 0;
  return e;
}

}  // namespace

// ctcd_stream_save for this stream (`committed`: the labels it has committed so far; the twin does not count them): compacts, then
// writes the image to out (cap bytes).  Returns the image's bytes (also when cap is too small: nothing is written then), or -1.
extern "C" long long ctcsnap_host_save(void *h, long long committed, unsigned char *out, long long cap) {
  using namespace ctcbeam;
  namespace sn = ctcsnap;
  CompactStream &c = *(CompactStream *)h;
  PeekStream &s = *c.s;
  const int live = compact(c);
  if (live < 0) return -1;
  const int M = s.frames > 0 ? live : 1, lm = s.lm ? 1 : 0;
  const size_t words = sn::snapshot_words(s.beam, lm, M);
  if ((long long)(words * 4) > cap || !out) return (long long)(words * 4);
  std::vector<int> img(words + 4, 0x5a5a5a5a);
  HostX x;
  const sn::SnapMeta m{(long long)s.frames, committed, lm ? sn::scorer_fingerprint(s.hs) : 0ull, s.V, lm ? sn::SNAP_SCORER_BUILTIN : sn::SNAP_SCORER_NONE};
  sn::snapshot_export(x, s.beam, M, m, s.hdr.data(), s.arrays.data(), s.pool.data(), s.pool_up.data(), (int)s.pool.size(), img.data());
  for (size_t i = words; i < words + 4; ++i)
    if (img[i] != 0x5a5a5a5a) return -1;  // (the export wrote behind its image)
  memcpy(out, img.data(), words * 4);
  return (long long)(words * 4);
}

// snapshot_check against this stream's configuration (beam, labels, scorer).  Returns the SNAP_* code; *at: where.
extern "C" int ctcsnap_host_check(const void *h, const unsigned char *blob, long long bytes, long long *at) {
  const CompactStream &c = *(const CompactStream *)h;
  ctcsnap::SnapError err;
  const int code = ctcsnap::snapshot_check(blob, bytes < 0 ? 0 : (size_t)bytes, expect_of(*c.s), &err);
  if (at) *at = err.at;
  return code;
}

// ctcd_stream_restore into this stream, which must be fresh (nothing fed): the image is checked, and only then the stream's pool is
// cut for it -- max(frames_hint frames, 2 M nodes) -- and filled.  Returns 0 (*committed: the labels the saved stream had
// committed), the SNAP_* code of a refusal (the stream is unchanged), or -1 (the stream is not fresh).
extern "C" int ctcsnap_host_restore(void *h, const unsigned char *blob, long long bytes, int frames_hint, long long *committed) {
  using namespace ctcbeam;
  namespace sn = ctcsnap;
  namespace cc = ctccompact;
  CompactStream &c = *(CompactStream *)h;
  PeekStream &s = *c.s;
  if (s.frames != 0) return -1;
  const int code = sn::snapshot_check(blob, bytes < 0 ? 0 : (size_t)bytes, expect_of(s), nullptr);
  if (code != sn::SNAP_OK) return code;
  sn::SnapInfo in;
  (void)sn::snapshot_info(blob, (size_t)bytes, &in);
  std::vector<int> img((size_t)bytes / 4);
  memcpy(img.data(), blob, (size_t)bytes);
  const long long hint = frames_hint > 0 ? frames_hint : 1024, for_2m = (2LL * in.nodes - 1 + s.beam - 1) / s.beam;
  c.hint_frames = hint;
  resize_pool(c, hint > for_2m ? hint : for_2m, 0);
  for (int &v : s.pool_up) v = 0x5a5a5a5a;  // (what the import must not rely on: a fresh device block is not zeroed either)
  const size_t head_ints = (size_t)SH_WORDS + (size_t)kStateArraysLm * s.beam;
  std::vector<int> head(head_ints, 0x5a5a5a5a);
  HostX x;
  sn::snapshot_import(x, img.data(), head.data(), head_ints, s.pool.data(), s.pool_up.data(), (int)s.pool.size());
  for (size_t i = 0; i < (size_t)SH_WORDS; ++i) s.hdr[i] = head[i];
  for (size_t i = 0; i < s.arrays.size(); ++i) s.arrays[i] = head[SH_WORDS + i];
  // (the express words behind the image's nodes stay as they are: never read before they are written, and undefined in a fresh device block)
  s.frames = (int)in.frames;
  if (in.frames > 0) { c.base_nodes = in.nodes; c.base_frames = in.frames; }
  if (committed) *committed = in.committed;
  return 0;
}

// ctcd_snapshot_info: out[0..9] = version, beam, labels, scorer kind, nodes, arrays, frames, committed, fingerprint, bytes
extern "C" int ctcsnap_host_info(const unsigned char *blob, long long bytes, unsigned long long *out) {
  ctcsnap::SnapInfo in;
  const int code = ctcsnap::snapshot_info(blob, bytes < 0 ? 0 : (size_t)bytes, &in);
  if (code != ctcsnap::SNAP_OK) return code;
  out[0] = (unsigned long long)in.version; out[1] = (unsigned long long)in.beam; out[2] = (unsigned long long)in.labels;
  out[3] = (unsigned long long)in.scorer_kind; out[4] = (unsigned long long)in.nodes; out[5] = (unsigned long long)in.arrays;
  out[6] = (unsigned long long)in.frames; out[7] = (unsigned long long)in.committed; out[8] = in.fingerprint; out[9] = in.bytes;
  return 0;
}

extern "C" unsigned long long ctcsnap_host_fingerprint(const void *h) {
  const PeekStream &s = *((const CompactStream *)h)->s;
  return s.lm ? ctcsnap::scorer_fingerprint(s.hs) : 0ull;
}

extern "C" const char *ctcsnap_host_error_name(int code) { return ctcsnap::snapshot_error_name(code); }
