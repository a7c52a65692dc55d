// CPU check of the host half of the dense MFMA element kernels (palace_amd/csrc/pa_dense_host.hpp) against a plain model of
// what the kernels of pa_dense.hip decode: for every (block, dof slot s, lane) a kernel reads dof 4 s + kq (kq = lane >> 4) of
// element lane & 15 of the block; its A operands come from the fragments Tf / Tt or from the resident copy L.  Then a sweep of
// the plan (PT, S, fit tests, launch bytes, list rule), printed for tests/test_dense_host.py to compare with tests/dense_cases.py.
// Built and run by tests/test_dense_host.py (g++, no GPU).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>

#include "pa_dense_host.hpp"

using namespace pa;
using namespace pa::densehost;

static int g_fail = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      if (g_fail++ < 20) {                    \
        std::printf("FAIL %s: ", #cond);      \
        std::printf(__VA_ARGS__);             \
        std::printf("\n");                    \
      }                                       \
    }                                         \
  } while (0)

// ---- the kernels' decode paths ---------------------------------------------------------------------------------------------------
// co_field / co_field_pk of pa_dense.hip (the shifts on the unsigned pattern: the same bits)
static double co_field(int c, int k) { return (double)((int32_t)((uint32_t)c << (30 - 2 * k)) >> 30); }
static double co_field_pk(unsigned w, int odd, int k) { return (double)((int32_t)(w << (30 - 2 * k - 16 * odd)) >> 30); }
// ye_pos of pa_dense.hip: (dof slot s, lane) inside a block's E-vector
static int ye_pos(int rows, int KP, int s, int lane) { return rows ? (lane & 15) * (4 * KP) + 4 * s + (lane >> 4) : s * 64 + lane; }

struct Restriction {
  int ne, P, lsize;
  std::vector<int32_t> off;
  std::vector<uint8_t> ori;
  std::vector<int8_t> cor;
  pa_restriction_desc desc() const {
    return {ne, P, lsize, off.data(), ori.empty() ? nullptr : ori.data(), cor.empty() ? nullptr : cor.data()};
  }
};
// kind 0 plain, 1 signed, 2 curl-oriented (any tridiagonal rows with entries -1, 0, 1)
static Restriction make_restriction(int ne, int P, int kind, std::mt19937 &rng) {
  Restriction R{ne, P, std::max(P + 3, ne * P / 2), {}, {}, {}};
  std::vector<int32_t> dofs(R.lsize);
  std::iota(dofs.begin(), dofs.end(), 0);
  for (int e = 0; e < ne; e++) {
    std::shuffle(dofs.begin(), dofs.end(), rng);
    R.off.insert(R.off.end(), dofs.begin(), dofs.begin() + P);
  }
  if (kind == 1)
    for (int k = 0; k < ne * P; k++) R.ori.push_back(rng() & 1);
  if (kind == 2)
    for (int k = 0; k < 3 * ne * P; k++) R.cor.push_back((int8_t)((int)(rng() % 3) - 1));
  return R;
}

static void check_index(const DensePlan &p, const Restriction &R) {
  const pa_restriction_desc r = R.desc();
  std::vector<int32_t> idx;
  std::vector<uint16_t> co;
  std::vector<uint32_t> co2;
  build_index(p, r, idx, co, co2);
  const int P = p.P, KP = p.KP;
  CHECK(idx.size() == (size_t)p.nb * KP * 64 && co.size() == (R.cor.empty() ? 0 : idx.size()) && co2.size() == co.size() / 2,
        "sizes P %d ne %d", P, p.ne);
  auto T = [&](int e, int d, int k) { return (d < 0 || d >= P) ? 0.0 : (double)R.cor[3 * ((size_t)e * P + d) + k]; };
  for (int b = 0; b < p.nb; b++)
    for (int s = 0; s < KP; s++)
      for (int lane = 0; lane < 64; lane++) {
        const int e = kEB * b + (lane & 15), d = 4 * s + (lane >> 4);
        const bool live = e < p.ne && d < P;
        const size_t at = ((size_t)b * KP + s) * 64 + lane;
        int32_t want = kEssBit;
        if (live) want = (!R.ori.empty() && R.ori[(size_t)e * P + d]) ? -1 - R.off[(size_t)e * P + d] : R.off[(size_t)e * P + d];
        CHECK(idx[at] == want, "idx P %d ne %d b %d s %d lane %d: %d, expected %d", P, p.ne, b, s, lane, idx[at], want);
        CHECK(at == block_pos(false, KP, e, d), "block_pos by dof rows");
        CHECK((size_t)b * KP * 64 + ye_pos(1, KP, s, lane) == block_pos(true, KP, e, d), "block_pos by element rows");
        if (R.cor.empty()) continue;
        // row d of T_e {sub, main, super}, then column d {T[d-1][d], T[d+1][d]}; padding decodes to zeros
        const double want_f[5] = {live ? T(e, d, 0) : 0.0, live ? T(e, d, 1) : 0.0, live ? T(e, d, 2) : 0.0, live ? T(e, d - 1, 2) : 0.0,
                                  live ? T(e, d + 1, 0) : 0.0};
        const unsigned w2 = co2[((size_t)b * (KP / 2) + s / 2) * 64 + lane];
        for (int k = 0; k < 5; k++) {
          CHECK(co_field(co[at], k) == want_f[k], "co P %d e %d d %d field %d", P, e, d, k);
          CHECK(co_field_pk(w2, s & 1, k) == want_f[k], "co2 P %d e %d d %d field %d", P, e, d, k);
        }
      }
}

static void check_transpose(const DensePlan &p, const Restriction &R) {
  const pa_restriction_desc r = R.desc();
  std::vector<int32_t> tptr, ted, tent;
  build_transpose(p, r, tptr, ted);
  const int P = p.P, KP = p.KP;
  CHECK((int)tptr.size() == R.lsize + 1 && tptr[0] == 0 && tptr[R.lsize] == p.ne * P && (int)ted.size() == p.ne * P, "tptr ends");
  for (int rows = 0; rows < 2; rows++) {
    build_tent(p, r, ted, rows != 0, tent);
    size_t seen = 0;
    for (int dof = 0; dof < R.lsize; dof++) {
      int last = -1;
      for (int k = tptr[dof]; k < tptr[dof + 1]; k++, seen++) {
        const int e = ted[k] / P, j = ted[k] % P;
        CHECK(R.off[ted[k]] == dof && ted[k] > last, "copies of dof %d: every one once, in element order", dof);
        last = ted[k];
        const int lane = (j & 3) * 16 + e % kEB;  // the lane that stores dof j = 4 s + kq of element e
        const int pos = (e / kEB) * KP * 64 + ye_pos(rows, KP, j >> 2, lane);
        const bool flip = !R.ori.empty() && R.ori[ted[k]];
        CHECK(tent[k] == (flip ? -1 - pos : pos), "tent rows %d dof %d copy %d: %d, position %d flip %d", rows, dof, k, tent[k], pos, flip);
      }
    }
    CHECK(seen == (size_t)p.ne * P, "every copy listed");
  }
  const std::vector<int32_t> rows = touched_rows(tptr);
  std::vector<char> has(R.lsize, 0);
  for (int32_t o : R.off) has[o] = 1;
  size_t n = 0;
  for (int d = 0; d < R.lsize; d++)
    if (has[d]) CHECK(n < rows.size() && rows[n++] == d, "row list: dof %d", d);
  CHECK(n == rows.size(), "row list length");
}

// What the operand reads expect.  A field of nc components has 16 nc rows per chunk of 16 points: row 4 pi + kq, pi = 4 gl + ... the
// pair (point group gl, component k) = (pi / nc, pi % nc), is component cb + k at point 16 c + 4 gl + kq (the C layout of the
// forward product: lane kq, register pi & 3 of tile pi >> 2 -- what D reads and what the transposed product takes as its B operand).
static void check_tables(const DensePlan &p, int mode, std::mt19937 &rng) {
  const ModeComps m = mode_comps(mode);
  const int P = p.P, Q = p.Q, KP = p.KP, PT = p.PT, nct = m.nct();
  std::uniform_real_distribution<double> U(0.5, 1.5);  // (no zero entries: a zero is padding)
  std::vector<double> interp((size_t)m.nci * Q * P), deriv((size_t)m.ncd * Q * P);
  for (double &v : interp) v = U(rng);
  for (double &v : deriv) v = U(rng);
  auto entry = [&](int comp, int q, int d) {
    if (q >= Q || d >= P) return 0.0;
    return comp < m.nci ? interp[((size_t)comp * Q + q) * P + d] : deriv[((size_t)(comp - m.nci) * Q + q) * P + d];
  };
  const Tables T{interp.data(), deriv.data(), m, P, Q};
  std::vector<double> Tf, Tt, L;
  build_fragments(p, T, Tf, Tt);
  build_resident(p, T, L);
  CHECK(Tf.size() == (size_t)p.nch * KP * nct * 64 && Tt.size() == (size_t)p.nch * 4 * nct * PT * 64 && L.size() == (size_t)p.rows * p.S,
        "table sizes mode %d P %d Q %d", mode, P, Q);
  CHECK(p.rows == p.nch * nct * 16 && p.S == resident_stride(PT) && p.S >= 16 * PT, "rows and stride");
  const int nf = (m.nci > 0) + (m.ncd > 0);
  size_t of = 0, ot = 0;  // the kernels walk the fragments chunk by chunk, field by field
  std::vector<char> touched(L.size(), 0);
  for (int c = 0; c < p.nch; c++) {
    int cb = 0;
    for (int f = 0; f < nf; f++) {
      const int nc = nf == 2 ? (f == 0 ? m.nci : m.ncd) : nct;
      const size_t row0 = (size_t)16 * (nct * c + cb);  // first resident row of the field: r0 = 16 NCT c, field 1 after 16 NC0 rows
      auto expect = [&](int row, int d) { return entry(cb + (row >> 2) % nc, 16 * c + 4 * ((row >> 2) / nc) + (row & 3), d); };
      // forward: tile t, lane (i = lane & 15, kq = lane >> 4) holds A[16 t + i][4 s + kq]
      for (int s = 0; s < KP; s++)
        for (int t = 0; t < nc; t++)
          for (int lane = 0; lane < 64; lane++) {
            const int i = lane & 15, kq = lane >> 4;
            const double want = expect(16 * t + i, 4 * s + kq);
            const size_t at = (row0 + 16 * t + i) * p.S + 4 * s + kq;
            CHECK(Tf[of + ((size_t)s * nc + t) * 64 + lane] == want, "Tf mode %d c %d f %d s %d t %d lane %d", mode, c, f, s, t, lane);
            CHECK(L[at] == want, "L forward mode %d c %d f %d s %d t %d lane %d", mode, c, f, s, t, lane);
            touched[at] = 1;
          }
      // transposed: row group pi, dof tile pt, lane (i, kq) holds A^T[16 pt + i][4 pi + kq]
      for (int pi = 0; pi < 4 * nc; pi++)
        for (int pt = 0; pt < PT; pt++)
          for (int lane = 0; lane < 64; lane++) {
            const int i = lane & 15, kq = lane >> 4;
            const double want = expect(4 * pi + kq, 16 * pt + i);
            CHECK(Tt[ot + ((size_t)pi * PT + pt) * 64 + lane] == want, "Tt mode %d c %d f %d pi %d pt %d lane %d", mode, c, f, pi, pt, lane);
            CHECK(L[(row0 + 4 * pi + kq) * p.S + 16 * pt + i] == want, "L transposed mode %d c %d f %d pi %d pt %d lane %d", mode, c, f, pi, pt, lane);
          }
      of += (size_t)KP * nc * 64, ot += (size_t)4 * nc * PT * 64, cb += nc;
    }
  }
  CHECK(of == Tf.size() && ot == Tt.size(), "fragment walk ends");
  for (size_t k = 0; k < L.size(); k++)
    if (!touched[k]) CHECK(L[k] == 0.0, "L stride padding at %zu", k);
  // zero exactly outside P x Q: as many non-zero entries as the tables have
  const size_t nnz = (size_t)nct * Q * P;
  CHECK((size_t)std::count_if(Tf.begin(), Tf.end(), [](double v) { return v != 0.0; }) == nnz, "Tf non-zeros");
  CHECK((size_t)std::count_if(Tt.begin(), Tt.end(), [](double v) { return v != 0.0; }) == nnz, "Tt non-zeros");
  CHECK((size_t)std::count_if(L.begin(), L.end(), [](double v) { return v != 0.0; }) == nnz, "L non-zeros");
  double chk = 0.0;
  for (size_t i = 0; i < interp.size(); i++) chk += interp[i] * (double)(1 + i % 1021);
  CHECK(table_checksum(interp.data(), interp.size()) == chk && table_checksum(nullptr, 5) == 0.0, "checksum");
}

static void check_small_things() {
  // the component table against the QFunctions' inputs
  for (int mode = 0; mode < kNumModes; mode++) {
    const ModeComps m = mode_comps(mode);
    CHECK(m.nf() >= 1 && m.nc(0) + (m.nf() == 2 ? m.nc(1) : 0) == m.nct() && m.cb(0) == 0, "fields of mode %d", mode);
  }
  CHECK(mode_of(PA_FE_HCURL, PA_QF_HDIVMASS_33, 3, 3) == MODE_CURLMASS && mode_of(PA_FE_H1, PA_QF_H1_1, 1, 3) == MODE_MASS &&
            mode_of(PA_FE_HCURL, PA_QF_HDIVMASS_32, 2, 3) == MODE_CURLMASS2,
        "mode_of");
  // symmetric coefficients
  CHECK(coeff_symmetric(3, {1, 2, 3, 2, 4, 5, 3, 5, 6}) && !coeff_symmetric(3, {1, 2, 3, 2, 4, 5, 3, 7, 6}) &&
            coeff_symmetric(2, {1, 2, 2, 3}) && !coeff_symmetric(2, {1, 2, 4, 3}) && coeff_symmetric(1, {7}),
        "coeff_symmetric");
  // the alias: RT mass in 3-D takes the curl-curl arithmetic with the values in the place of the curl; the pair in 3-D swaps
  DenseAlias a = resolve_alias(PA_FE_HDIV, PA_QF_HDIV_33, 33, PA_EVAL_INTERP, PA_EVAL_INTERP, {true, false}, false);
  CHECK(a.fe_type == PA_FE_HCURL && a.qf == PA_QF_HDIV_33 && a.trial_ops == PA_EVAL_CURL && !a.contra && a.interp == kNoTable &&
            a.deriv == kInterpTable,
        "alias: mass 33");
  a = resolve_alias(PA_FE_HDIV, PA_QF_L2MASS_33, 33, PA_EVAL_INTERP | PA_EVAL_DIV | PA_EVAL_WEIGHT, PA_EVAL_INTERP | PA_EVAL_DIV,
                    {true, true}, false);
  CHECK(a.fe_type == PA_FE_H1 && a.qf == PA_QF_HCURLMASS_33 && a.contra && a.interp == kDerivTable && a.deriv == kInterpTable,
        "alias: pair 33");
  a = resolve_alias(PA_FE_HDIV, PA_QF_HDIV_32, 32, PA_EVAL_INTERP, PA_EVAL_INTERP, {true, false}, false);
  CHECK(a.fe_type == PA_FE_HCURL && a.qf == PA_QF_HCURL_32 && a.contra && a.interp == kInterpTable, "alias: mass 32");
  a = resolve_alias(PA_FE_H1, PA_QF_H1_1, 33, 4, 4, {true, false}, true);
  CHECK(a.fe_type == PA_FE_H1 && a.qf == PA_QF_H1_1 && a.contra && a.trial_ops == 4, "no alias");
  bool threw = false;
  try {
    resolve_alias(PA_FE_HDIV, PA_QF_L2_1, 21, PA_EVAL_DIV, PA_EVAL_DIV, {false, true}, false);
  } catch (const std::exception &e) {
    threw = std::string(e.what()).find("H(div) elements: the div-div operator takes the divergence table") == 0;
  }
  CHECK(threw, "alias: div-div on a line is refused");
  // contexts: l2mass_33 has the matrix first and hands it to c1
  const CtxLayout l = ctx_layout(MODE_DIFFMASS, true, 3), l2 = ctx_layout(MODE_CURLMASS2, false, 2), l3 = ctx_layout(MODE_DIFFMASS1, true, 3);
  CHECK(l.n == 2 && l.part[0].dim == 3 && l.part[0].slot == 1 && l.part[1].dim == 1 && l.part[1].slot == 0, "contexts of l2mass_33");
  CHECK(l2.n == 2 && l2.part[0].dim == 2 && l2.part[0].slot == 0 && l2.part[1].dim == 1 && l2.part[1].slot == 1, "contexts of hdivmass_22");
  CHECK(l3.n == 2 && l3.part[0].dim == 3 && l3.part[0].slot == 0 && l3.part[1].dim == 1, "contexts of l2mass_31");
}

int main() {
  std::mt19937 rng(20240607);
  check_small_things();
  const int modes[] = {MODE_MASS, MODE_CURLMASS, MODE_CURLMASS2};
  for (int P : {13, 16, 29, 97})
    for (int ne : {1, 16, 17}) {
      const DensePlan pe = make_plan(ne, P, 5, 16, mode_comps(MODE_MASS));
      for (int kind = 0; kind < 3; kind++) {
        const Restriction R = make_restriction(ne, P, kind, rng);
        check_index(pe, R);
        check_transpose(pe, R);
      }
      for (int Q : {5, 16, 17})
        for (int mode : modes) check_tables(make_plan(ne, P, Q, (Q + 15) / 16 * 16, mode_comps(mode)), mode, rng);
    }
  // ---- the plan, for the Python side: every PT, 1 to 6 components, 1 to 400 points, with and without the curl-oriented restriction
  for (int P = 1; P <= 145; P++) std::printf("pt %d %d\n", P, dense_pt(P));
  const int res_waves = 8, aff_waves = 12;  // kResWaves, kAffWaves of pa_dense.hip
  for (int PT : kPT)
    for (int nct = 1; nct <= 6; nct++)
      for (int Q = 1; Q <= 400; Q++)
        for (int curl = 0; curl < 2; curl++) {
          const DensePlan p = make_plan(16, 16 * PT, Q, (Q + 15) / 16 * 16, ModeComps{0, nct});
          std::printf("plan %d %d %d %d %d %d %d %d %zu %zu\n", PT, nct, Q, curl, p.PT, p.S, (int)resident_fits(p, curl != 0, res_waves),
                      (int)affine_fits(p, curl != 0, aff_waves), resident_launch_bytes(p.Q4, p.rows, p.PT, curl != 0, res_waves),
                      resident_launch_bytes(p.Q4, p.rows, p.PT, curl != 0, aff_waves));
        }
  for (int nb = 1; nb <= 40; nb++)
    for (int na = 0; na <= nb; na++) std::printf("lists %d %d %d\n", na, nb, (int)use_block_lists(na, nb));
  if (g_fail) std::printf("%d checks failed\n", g_fail);
  return g_fail ? 1 : 0;
}
