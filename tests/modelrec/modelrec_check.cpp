// TEST INFRASTRUCTURE ONLY -- what smj_load_model (csrc/smj_model_load.h) makes of a model blob, printed one item per line for
// tests/test_model_records.py: the return code and error text, the chosen variant, every scalar of DevModel, the word count and SHA-256
// of every table it derives, one SHA-256 over the tables it copies, and the values of the layout enums.  The capacities are those of
// the build table's rows (tests/routing/desc_probe.inc, one probe per tag), offered as smj_create offers them; `--tag <tag>` loads
// against that build's row alone, as smj_create loads the escalation model.  `--dump <table>` prints one table's words instead.
//   modelrec_check <blob> [--tag <tag>] [--dump <table>]
#include <stdio.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../host_uploader.h"
#include "smj_model_load.h"
#include "smj_variants.h"

#define X(tag) extern const SmjBuildDesc probe_product_##tag;
SMJ_BUILDS(X)
#undef X
static const SmjBuildDesc* const builds[SMJ_B_COUNT] = {
#define X(tag) &probe_product_##tag,
    SMJ_BUILDS(X)
#undef X
};

struct Sha256 {   // FIPS 180-4
  uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
  unsigned char buf[64];
  uint64_t len = 0;
  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const unsigned char* p) {
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
        0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
        0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
        0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
        0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
        0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t w[64], s[8];
    for (int i = 0; i < 16; i++) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | p[4 * i + 3];
    for (int i = 16; i < 64; i++)
      w[i] = w[i - 16] + (rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)) + w[i - 7] + (rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10));
    memcpy(s, h, sizeof s);
    for (int i = 0; i < 64; i++) {
      const uint32_t t1 = s[7] + (rotr(s[4], 6) ^ rotr(s[4], 11) ^ rotr(s[4], 25)) + ((s[4] & s[5]) ^ (~s[4] & s[6])) + K[i] + w[i];
      const uint32_t t2 = (rotr(s[0], 2) ^ rotr(s[0], 13) ^ rotr(s[0], 22)) + ((s[0] & s[1]) ^ (s[0] & s[2]) ^ (s[1] & s[2]));
      for (int q = 7; q > 0; q--) s[q] = s[q - 1];
      s[4] += t1;
      s[0] = t1 + t2;
    }
    for (int q = 0; q < 8; q++) h[q] += s[q];
  }
  void add(const void* data, size_t n) {
    const unsigned char* p = (const unsigned char*)data;
    for (size_t i = 0; i < n; i++) {
      buf[len++ % 64] = p[i];
      if (len % 64 == 0) block(buf);
    }
  }
  std::string hex() {
    const uint64_t bits = len * 8;
    const unsigned char one = 0x80, zero = 0;
    add(&one, 1);
    while (len % 64 != 56) add(&zero, 1);
    for (int q = 7; q >= 0; q--) { const unsigned char c = (unsigned char)(bits >> (8 * q)); add(&c, 1); }
    char out[65];
    for (int q = 0; q < 8; q++) snprintf(out + 8 * q, 9, "%08x", h[q]);
    return out;
  }
};

// every scalar of DevModel (csrc/smj_model.h), ints and floats
#define MODEL_INTS(X)                                                                                                                   \
  X(nq) X(nv) X(nu) X(nbody) X(njnt) X(ngeom) X(nsite) X(neq) X(npair) X(nlevel) X(nfric) X(nlimit) X(nplanepair) X(nldl) X(nlidar)      \
  X(imu_site) X(ngc) X(nroot) X(nkey) X(ncgeom) X(nconvpair) X(njump) X(maxsubtree) X(iterations) X(warmstart) X(pgs_fixed_iter)        \
  X(max_con_pair) X(solver) X(ls_iterations) X(convex_pairs) X(pgs_island_stop) X(qcqp_exact) X(pgs_dual_ws) X(sep_cache)               \
  X(manifold_cache) X(multi_serial) X(pgs_cap) X(row_limit) X(multiccd) X(nsat) X(nq_all) X(nv_all) X(nbody_all) X(nfric_main)          \
  X(nlimit_main) X(nsgeom) X(nstatpair) X(grid_dim[0]) X(grid_dim[1]) X(grid_dim[2])
#define MODEL_FLOATS(X)                                                                                                                 \
  X(grad_noise) X(ls_tolerance) X(timestep) X(gravity[0]) X(gravity[1]) X(gravity[2]) X(impratio) X(tolerance) X(meaninertia)           \
  X(lidar_cutoff) X(grid_org[0]) X(grid_org[1]) X(grid_org[2]) X(grid_h) X(grid_margin)
// the tables the loader derives, each found through its DevModel pointer
#define MODEL_DERIVED(X)                                                                                                                \
  X(k_lanerec) X(k_pprec) X(k_cgrec) X(k_rowrec) X(k_cprec) X(k_sgrec) X(k_sprec) X(k_spair) X(k_grid_adr) X(k_grid_list) X(k_sg_cell)   \
  X(k_sg_bound) X(k_sgw) X(k_satrec)

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const char *tag = nullptr, *dump = nullptr;
  for (int a = 2; a + 1 < argc; a += 2) {
    if (!strcmp(argv[a], "--tag")) tag = argv[a + 1];
    else if (!strcmp(argv[a], "--dump")) dump = argv[a + 1];
    else return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<unsigned char> blob;
  unsigned char buf[1 << 16];
  for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + n);
  fclose(f);

  std::vector<SmjCaps> caps;
  std::vector<const char*> names;
  if (tag) {
    for (int i = 0; i < SMJ_B_COUNT; i++)
      if (!strcmp(builds[i]->tag, tag)) { caps.push_back(builds[i]->caps); names.push_back(builds[i]->tag); }
    if (caps.empty()) { fprintf(stderr, "no build %s\n", tag); return 2; }
  } else {
    for (int v = 0; v < SMJ_NVARIANTS; v++) { caps.push_back(builds[smj_variants[v].newton]->caps); names.push_back(smj_variants[v].name); }
  }
  std::vector<void*> keep;
  std::map<const void*, size_t> bytes;
  HostUploader up{&keep, &bytes};
  DevModel m{};
  std::string err;
  int chosen = -1;
  const int rc = smj_load_model(blob.data(), blob.size(), m, up, err, caps.data(), (int)caps.size(), &chosen);
  auto size_of = [&](const void* p) { return p ? bytes.at(p) : (size_t)0; };
  if (dump) {
    const void* p = nullptr;
#define X(n) if (!strcmp(dump, #n)) p = m.n;
    MODEL_DERIVED(X) SMJ_MODEL_I32(X) SMJ_MODEL_F32(X)
#undef X
    if (rc || !p) { fprintf(stderr, "no table %s (rc %d %s)\n", dump, rc, err.c_str()); return 1; }
    for (size_t i = 0; i < size_of(p) / 4; i++) printf("%d\n", ((const int*)p)[i]);
  } else {
    printf("rc %d\nerr %s\nvariant %s\n", rc, err.c_str(), rc ? "-" : names[chosen]);
    if (!rc) {
#define X(n) printf(#n " %d\n", m.n);
      MODEL_INTS(X)
#undef X
#define X(n) { int b; memcpy(&b, &m.n, 4); printf(#n " 0x%08x\n", (unsigned)b); }
      MODEL_FLOATS(X)
#undef X
#define X(n) { Sha256 s; s.add(m.n, size_of(m.n)); printf(#n " %zu %s\n", size_of(m.n) / 4, m.n ? s.hex().c_str() : "null"); }
      MODEL_DERIVED(X)
#undef X
      Sha256 si, sf;
#define X(n) { const uint32_t w = (uint32_t)(size_of(m.n) / 4); si.add(&w, 4); si.add(m.n, size_of(m.n)); }
      SMJ_MODEL_I32(X)
#undef X
#define X(n) { const uint32_t w = (uint32_t)(size_of(m.n) / 4); sf.add(&w, 4); sf.add(m.n, size_of(m.n)); }
      SMJ_MODEL_F32(X)
#undef X
      printf("SMJ_MODEL_I32 %s\nSMJ_MODEL_F32 %s\n", si.hex().c_str(), sf.hex().c_str());
    }
    // the layouts (csrc/smj_model.h); SMJ_LR_ACT / SMJ_LR_STRIDE are functions of the mass-matrix slots per lane (5 and 8 in the table)
#define E(n) printf(#n " %d\n", (int)(n));
    E(SMJ_LR_KIN) E(SMJ_LR_BODY) E(SMJ_LR_DOF) E(SMJ_LR_ENT) E(smj_lr_act(5)) E(smj_lr_stride(5)) E(smj_lr_act(8)) E(smj_lr_stride(8))
    E(SMJ_SR_BODY) E(SMJ_SR_JTYPE) E(SMJ_SR_QADR) E(SMJ_SR_DADR) E(SMJ_SR_NDOF) E(SMJ_SR_JNT) E(SMJ_SR_F) E(SMJ_SR_POS) E(SMJ_SR_QUAT)
    E(SMJ_SR_JPOS) E(SMJ_SR_JAXIS) E(SMJ_SR_Q0) E(SMJ_SR_INL) E(SMJ_SR_ARM) E(SMJ_SR_DAMP) E(SMJ_SR_STIFF) E(SMJ_SR_SPRING)
    E(SMJ_SR_GCMASS) E(SMJ_SR_GCIPOS) E(SMJ_SR_STRIDE) E(SMJ_CP_STRIDE) E(SMJ_RR_STRIDE) E(SMJ_PP_STRIDE) E(SMJ_CG_STRIDE)
    E(SMJ_SAT_I_STRIDE) E(SMJ_SAT_F_STRIDE) E(SMJ_SGW_STRIDE) E(SMJ_SGB_STRIDE)
#undef E
  }
  for (void* p : keep) free(p);
  return 0;
}
