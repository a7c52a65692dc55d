// Host half of the dense MFMA element kernels (pa_dense.hip): everything make_dense_sub decides or encodes before anything reaches
// the device -- the mode of a block, the H(div) alias, the coefficient-context layout, the plan (sizes, fit tests, LDS bytes) and
// the builders of the index words, the transpose map and the table fragments.  Plain C++ without HIP so that
// tests/test_dense_host.py can compile it with g++ and check it against a CPU model of what the kernels decode.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/palace_amd.h"
#include "pa_stream_host.hpp"  // kEssBit

// (the text of PA_REQUIRE, pa_internal.hpp, without its HIP header)
#define PA_DENSE_REQUIRE(cond, msg)                                                 \
  do {                                                                              \
    if (!(cond)) throw std::runtime_error(std::string(msg) + " [" #cond "]");       \
  } while (0)

namespace pa {
namespace densehost {

constexpr int kEB = 16;  // elements per block (N of the MFMA tile)

enum DenseMode {
  MODE_CURL = 0,      // ND curl-curl              f_apply_hdiv_33 on curl u
  MODE_VMASS = 1,     // ND mass                   f_apply_hcurl_33 on u
  MODE_CURLMASS = 2,  // ND curl-curl + mass       f_apply_hdivmass_33
  MODE_DIFF = 3,      // H1 diffusion              f_apply_hcurl_33 on grad u
  MODE_DIFFMASS = 4,  // H1 diffusion + mass       f_apply_hcurlmass_33
  MODE_MASS = 5,      // H1 mass                   f_apply_h1_1
  // 2-D (fast path only: tables resident in LDS + packed D)
  MODE_CURL2 = 6,     // 2-D ND curl-curl          f_apply_l2_1 on the scalar curl (q_w input)
  MODE_VMASS2 = 7,    // 2-D ND mass               f_apply_hcurl_22
  MODE_CURLMASS2 = 8, // 2-D ND curl-curl + mass   f_apply_hdivmass_22 / _32
  MODE_DIFF2 = 9,     // 2-D H1 diffusion          f_apply_hcurl_22 / _32 on grad u
  MODE_DIFFMASS2 = 10, // 2-D H1 diffusion + mass   f_apply_hcurlmass_22 / _32
  // (MODE_MASS serves the 2-D and 1-D H1 mass too: f_apply_h1_1 only reads w detJ)
  // line elements (boundaries of plane problems, curves in space): every D is a scalar per point
  MODE_VMASS1 = 11,    // ND mass on a line         f_apply_hcurl_21 / _31
  MODE_DIFF1 = 12,     // H1 diffusion on a line    f_apply_hcurl_21 / _31 on du/dxi
  MODE_DIFFMASS1 = 13  // H1 diffusion + mass       f_apply_hcurlmass_21 / _31
};
constexpr int kNumModes = 14;

// Components of a mode: of the interp part (values) and of the curl / gradient part.  ModeTraits and FieldTraits of pa_dense.hip
// and every run-time lookup read this one table.
struct ModeComps {
  int nci, ncd;
  constexpr int nct() const { return nci + ncd; }
  // fields: the interp part if the mode has one, then the curl / gradient part
  constexpr int nf() const { return (nci > 0 ? 1 : 0) + (ncd > 0 ? 1 : 0); }
  constexpr int nc(int f) const { return nf() == 2 ? (f == 0 ? nci : ncd) : nct(); }  // components of field f
  constexpr int cb(int f) const { return (nf() == 2 && f == 1) ? nci : 0; }            // ... and the number of components before it
};
constexpr ModeComps kModeComps[kNumModes] = {{0, 3}, {3, 0}, {3, 3}, {0, 3}, {1, 3}, {1, 0}, {0, 1},
                                             {2, 0}, {2, 1}, {0, 2}, {1, 2}, {1, 0}, {0, 1}, {1, 1}};
constexpr ModeComps mode_comps(int mode) { return kModeComps[mode]; }
constexpr int packed_sym(int n) { return n == 3 ? 6 : (n == 2 ? 3 : n); }  // entries of a packed symmetric n x n D

inline int mode_of(int fe_type, int qf, int dim, int sdim) {
  if (dim == 1) {  // line elements in the plane (21) or in space (31)
    const int q_vec = sdim == 3 ? PA_QF_HCURL_31 : PA_QF_HCURL_21, q_pair = sdim == 3 ? PA_QF_HCURLMASS_31 : PA_QF_HCURLMASS_21;
    if (fe_type == PA_FE_HCURL && qf == q_vec) return MODE_VMASS1;
    if (fe_type == PA_FE_H1 && qf == PA_QF_H1_1) return MODE_MASS;
    if (fe_type == PA_FE_H1 && qf == q_vec) return MODE_DIFF1;
    if (fe_type == PA_FE_H1 && qf == q_pair) return MODE_DIFFMASS1;
    throw std::runtime_error("QFunction does not match a line element");
  }
  if (dim == 2) {  // the same applies for plane elements and for boundary elements in 3-D: only D differs (3x2 geometry)
    const bool bdr = sdim == 3;
    if (fe_type == PA_FE_HCURL) {
      if (qf == PA_QF_L2_1) return MODE_CURL2;
      if (qf == (bdr ? PA_QF_HCURL_32 : PA_QF_HCURL_22)) return MODE_VMASS2;
      if (qf == (bdr ? PA_QF_HDIVMASS_32 : PA_QF_HDIVMASS_22)) return MODE_CURLMASS2;
      throw std::runtime_error(bdr ? "QFunction does not match an H(curl) boundary element" : "QFunction does not match a 2-D H(curl) element");
    }
    if (qf == PA_QF_H1_1) return MODE_MASS;
    if (qf == (bdr ? PA_QF_HCURL_32 : PA_QF_HCURL_22)) return MODE_DIFF2;
    if (qf == (bdr ? PA_QF_HCURLMASS_32 : PA_QF_HCURLMASS_22)) return MODE_DIFFMASS2;
    throw std::runtime_error(bdr ? "QFunction does not match an H1 boundary element" : "QFunction does not match a 2-D H1 element");
  }
  if (fe_type == PA_FE_HCURL) {
    if (qf == PA_QF_L2_1) return MODE_CURL2;  // (reached through the H(div) alias: div-div, a scalar derivative in 3-D)
    if (qf == PA_QF_HDIV_33) return MODE_CURL;
    if (qf == PA_QF_HCURL_33) return MODE_VMASS;
    if (qf == PA_QF_HDIVMASS_33) return MODE_CURLMASS;
  } else {
    if (qf == PA_QF_HCURL_33) return MODE_DIFF;
    if (qf == PA_QF_HCURLMASS_33) return MODE_DIFFMASS;
    if (qf == PA_QF_H1_1) return MODE_MASS;
  }
  throw std::runtime_error("QFunction does not match the element type");
}

// ---- the H(div) alias ----------------------------------------------------------------------------------------------------------
// H(div) elements run on the arithmetic of an existing mode: the tables change places, the D of the values takes the contravariant
// map (`contra`: AdjJt of the stored adj(J)^T / detJ, what f_apply_hdiv_* do first).
enum TableSrc { kNoTable = 0, kInterpTable = 1, kDerivTable = 2 };  // which of the caller's tables stands in a place
struct TablesGiven { bool interp, deriv; };
struct DenseAlias {
  int fe_type, qf;
  uint32_t trial_ops, test_ops;
  bool contra;
  TableSrc interp, deriv;  // what stands in the place of the value table and of the curl / gradient table
};
// d = 10 * sdim + dim.  Any other element type passes through as it came.
inline DenseAlias resolve_alias(int fe_type, int qf, int d, uint32_t trial_ops, uint32_t test_ops, const TablesGiven &b, bool contra) {
  if (fe_type != PA_FE_HDIV) return {fe_type, qf, trial_ops, test_ops, contra, kInterpTable, kDerivTable};
  const uint32_t t_ops = trial_ops & ~(uint32_t)PA_EVAL_WEIGHT, s_ops = test_ops & ~(uint32_t)PA_EVAL_WEIGHT;
  const uint32_t curl = PA_EVAL_CURL, val = PA_EVAL_INTERP, val_curl = PA_EVAL_INTERP | PA_EVAL_CURL,
                 val_grad = PA_EVAL_INTERP | PA_EVAL_GRAD;
  if (qf == PA_QF_L2_1) {
    // div-div (fem/integ/divdiv.cpp: Div | Weight, f_apply_l2_1 for single-component elements): the scalar-derivative
    // arithmetic of the 2-D curl-curl, c qw^2 / (w detJ), with the divergence table [Q][P] in the place of the curl table
    PA_DENSE_REQUIRE((d == 33 || d == 22 || d == 32) && t_ops == PA_EVAL_DIV && s_ops == PA_EVAL_DIV && b.deriv,
                     "H(div) elements: the div-div operator takes the divergence table with Div (| Weight)");
    return {PA_FE_HCURL, qf, curl, curl, false, kNoTable, kDerivTable};
  }
  const int q_mass = d == 33 ? PA_QF_HDIV_33 : d == 22 ? PA_QF_HDIV_22 : d == 32 ? PA_QF_HDIV_32 : d == 21 ? PA_QF_HDIV_21 : PA_QF_HDIV_31;
  const int q_pair = d == 33   ? PA_QF_L2MASS_33
                     : d == 22 ? PA_QF_L2MASS_22
                     : d == 32 ? PA_QF_L2MASS_32
                     : d == 21 ? PA_QF_L2MASS_21
                               : PA_QF_L2MASS_31;
  if (qf == q_mass) {
    PA_DENSE_REQUIRE(t_ops == PA_EVAL_INTERP && s_ops == PA_EVAL_INTERP && b.interp, "H(div) mass: Interp on the value table");
    // (fem/integ/vecfemass.cpp with an RT space: Interp + f_apply_hdiv_33) the arithmetic of the curl-curl operator with the
    // value table in the place of the curl table
    if (d == 33) return {PA_FE_HCURL, qf, curl, curl, false, kNoTable, kInterpTable};
    // plane, boundary and line elements (f_apply_hdiv_22 | _32 | _21 | _31): the vector mass of the geometry with the
    // contravariant map in the place of adjJt
    const int q_cov = d == 22 ? PA_QF_HCURL_22 : d == 32 ? PA_QF_HCURL_32 : d == 21 ? PA_QF_HCURL_21 : PA_QF_HCURL_31;
    return {PA_FE_HCURL, q_cov, val, val, true, kInterpTable, kDerivTable};
  }
  PA_DENSE_REQUIRE(qf == q_pair, "H(div) elements: the mass operator (Interp, hdiv_*), div-div (Div, l2_1) and div-div + mass "
                                 "(Interp | Div, l2mass_*) of the geometry's dimensions are supported");
  // DivDivMassIntegrator (fem/integ/divdivmass.cpp: Interp | Div | Weight, f_apply_l2mass_*; pair context: mass first)
  PA_DENSE_REQUIRE(t_ops == (PA_EVAL_INTERP | PA_EVAL_DIV) && s_ops == t_ops && b.interp && b.deriv,
                   "div-div + mass: value and divergence tables with Interp | Div (| Weight)");
  if (d == 22 || d == 32)  // the plane / boundary curl-curl + mass: two values, one scalar derivative
    return {PA_FE_HCURL, d == 22 ? PA_QF_HDIVMASS_22 : PA_QF_HDIVMASS_32, val_curl, val_curl, true, kInterpTable, kDerivTable};
  if (d == 33)  // diffusion + mass with the roles exchanged: one "value" (the divergence), three "derivatives" (the values)
    return {PA_FE_H1, PA_QF_HCURLMASS_33, val_grad, val_grad, true, kDerivTable, kInterpTable};
  // line elements: one value, one derivative -- the tables stay where they are
  return {PA_FE_H1, d == 21 ? PA_QF_HCURLMASS_21 : PA_QF_HCURLMASS_31, val_grad, val_grad, true, kInterpTable, kDerivTable};
}

// ---- the coefficient context(s) ------------------------------------------------------------------------------------------------
// The contexts of a block in the order they lie in the caller's blob: the dimension of each and whether it is the kernels' c0 or c1.
struct CtxPart { int dim, slot; };  // dim: 1 scalar, 3, or kCtxMat; slot 0: DenseSub::c0, 1: c1
struct CtxLayout { int n; CtxPart part[2]; };
constexpr int kCtxMat = 0;  // the material matrix of the space: 3 x 3 on boundary elements and curves in space, else 2 x 2
constexpr CtxLayout kCtxLayout[kNumModes] = {
    {1, {{3, 0}}},                  // CURL
    {1, {{3, 0}}},                  // VMASS
    {2, {{3, 0}, {3, 1}}},          // CURLMASS   hdivmass_33: mass context first
    {1, {{3, 0}}},                  // DIFF
    {2, {{1, 0}, {3, 1}}},          // DIFFMASS   hcurlmass_33: scalar mass context first
    {1, {{1, 0}}},                  // MASS
    {1, {{1, 0}}},                  // CURL2
    {1, {{kCtxMat, 0}}},            // VMASS2
    {2, {{kCtxMat, 0}, {1, 1}}},    // CURLMASS2
    {1, {{kCtxMat, 0}}},            // DIFF2
    {2, {{1, 0}, {kCtxMat, 1}}},    // DIFFMASS2
    {1, {{kCtxMat, 0}}},            // VMASS1
    {1, {{kCtxMat, 0}}},            // DIFF1
    {2, {{1, 0}, {kCtxMat, 1}}}};   // DIFFMASS1
// the div-div + mass pairs of H(div) elements (`contra`) that differ from the table:
constexpr CtxLayout kCtxL2Mass33 = {2, {{3, 1}, {1, 0}}};        // l2mass_33: the 3 x 3 mass coefficient first, then the scalar one
constexpr CtxLayout kCtxL2MassLine = {2, {{kCtxMat, 0}, {1, 1}}};  // l2mass_21 | _31: the mass matrix first, then the scalar one
inline CtxLayout ctx_layout(int mode, bool contra, int sdim) {
  CtxLayout l = contra && mode == MODE_DIFFMASS ? kCtxL2Mass33 : contra && mode == MODE_DIFFMASS1 ? kCtxL2MassLine : kCtxLayout[mode];
  for (int k = 0; k < l.n; k++)
    if (l.part[k].dim == kCtxMat) l.part[k].dim = sdim == 3 ? 3 : 2;  // boundary elements take the 3x3 material
  return l;
}
// the resident kernels read packed symmetric D: every dim x dim matrix of a context (column-major, back to back) symmetric?
inline bool coeff_symmetric(int dim, const std::vector<double> &mat) {
  if (dim == 2) {
    for (size_t k = 0; k + 4 <= mat.size(); k += 4)
      if (mat[k + 1] != mat[k + 2]) return false;
    return true;
  }
  if (dim != 3) return true;
  for (size_t k = 0; k + 9 <= mat.size(); k += 9)
    if (mat[k + 1] != mat[k + 3] || mat[k + 2] != mat[k + 6] || mat[k + 5] != mat[k + 7]) return false;
  return true;
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------
constexpr int kPT[] = {1, 2, 3, 4, 6, 9};  // 16 PT = the padded dof count of an element: the instantiated sizes
inline int dense_pt(int P) {               // 0: more than 144 dofs
  for (int v : kPT)
    if (P <= 16 * v) return v;
  return 0;
}
// row stride of the LDS-resident tables, 18 (mod 32) doubles (ResidentStride of pa_dense.hip)
constexpr int resident_stride(int PT) { return 16 * PT + ((PT & 1) ? 2 : 18); }
constexpr int round_up4(int Q) { return (Q + 3) / 4 * 4; }  // point stride of the packed q-data (DenseArgs::Q4)

struct DensePlan {
  int ne = 0, nb = 0, P = 0, Q = 0;  // the sizes it was made from; nb blocks of kEB elements
  int PT = 0, KP = 0;                // KP = 4 PT dof slots per lane
  int Qpad = 0, nch = 0, Q4 = 0;     // points padded to chunks of 16 (the geometry data's), chunks, points rounded up to 4 (q-data)
  int S = 0, rows = 0, ncq = 0;      // resident tables [rows][S]; q-data components
};
inline DensePlan make_plan(int ne, int P, int Q, int Qpad, ModeComps m) {
  DensePlan p;
  p.ne = ne, p.nb = (ne + kEB - 1) / kEB, p.P = P, p.Q = Q;
  p.PT = dense_pt(P), p.KP = 4 * p.PT;
  p.Qpad = Qpad, p.nch = Qpad / 16, p.Q4 = round_up4(Q);
  p.S = resident_stride(p.PT), p.rows = p.nch * m.nct() * 16, p.ncq = packed_sym(m.nci) + packed_sym(m.ncd);
  return p;
}
inline size_t num_slots(const DensePlan &p) { return (size_t)p.nb * p.KP * 64; }  // entries of idx, co and the E-vector

// Dynamic LDS a launch of the resident kernel asks for: the weight prefix, the tables and, for the curl-oriented restriction, the
// neighbour exchange of its `nw` waves.
inline size_t resident_launch_bytes(int Q4, int rows, int PT, bool curl, int nw) {
  return sizeof(double) * ((size_t)(Q4 + 31) / 32 * 32 + (size_t)rows * resident_stride(PT) + (curl ? (size_t)nw * 4 * PT * 64 : 0));
}
// What the fit test of the resident form counts: NOT the launch size -- the tables and the exchange of the curved form's waves,
// without the weight prefix -- against 150 KiB.  The 10 KiB up to the 160 KiB a launch may ask for hold the prefix it leaves out
// (tables that fit have fewer than 1100 rows, so fewer points than that: under 9 KiB of weights).
constexpr size_t kResidentFitLimit = 150 * 1024, kLaunchLimit = 160 * 1024;
inline size_t resident_fit_bytes(const DensePlan &p, bool curl, int res_waves) {
  return sizeof(double) * ((size_t)p.rows * p.S + (curl ? (size_t)res_waves * 4 * p.PT * 64 : 0));
}
// (PT <= 6: the resident kernel is not instantiated for 144 padded dofs -- a block of 97 to 144 dofs whose tables would fit,
// a one-component mode with few points, was given the resident form here and then refused at its first apply)
inline bool resident_fits(const DensePlan &p, bool curl, int res_waves) {
  return p.PT <= 6 && resident_fit_bytes(p, curl, res_waves) <= kResidentFitLimit;
}
// The affine form runs more waves, so its exchange space is larger: its test IS the launch size against the launch limit.
// (PT <= 3: larger blocks have no registers for the values kept across the block; one point leaves nothing to save)
inline bool affine_fits(const DensePlan &p, bool curl, int aff_waves) {
  return p.PT <= 3 && resident_launch_bytes(p.Q4, p.rows, p.PT, curl, aff_waves) <= kLaunchLimit && p.Q > 1;
}
// a mesh with curved parts: the affine blocks get the affine kernel through a list when they are a quarter of the blocks or more
inline bool use_block_lists(int n_affine, int nb) { return n_affine < nb && n_affine * 4 >= nb; }
// a block that touches few of the dofs adds its result through the list of the rows it has
inline bool few_rows(const DensePlan &p, int lsize) { return (size_t)p.ne * p.P * 4 < (size_t)lsize; }

// ---- E: index words and the transpose map ----------------------------------------------------------------------------------------
// (element e, local dof d) in the whole E-vector [nb][4 KP][16]: rows = false, [dof][element] (one 128-byte row per dof: what the
// kernels' lanes hold side by side; the index table always has these rows), rows = true: [element][dof]
inline size_t block_pos(bool rows, int KP, int e, int d) {
  const size_t blk = (size_t)(e / kEB) * 4 * KP * kEB;
  return rows ? blk + (size_t)(e % kEB) * 4 * KP + d : blk + (size_t)d * kEB + (e % kEB);
}

// idx: block-transposed signed index (oriented: < 0 => -(1 + dof) flipped), kEssBit on padding.  co (curl-oriented restriction
// only): 2-bit fields {sub, main, super} of row d of T_e and {T[d-1][d], T[d+1][d]} of column d; co2: the words of dof slots 2 s
// and 2 s + 1 of a lane in one register, [nb][KP / 2][64] (the resident kernel: half the loads and registers)
inline void build_index(const DensePlan &p, const pa_restriction_desc &r, std::vector<int32_t> &idx, std::vector<uint16_t> &co,
                        std::vector<uint32_t> &co2) {
  const int P = p.P, KP = p.KP;
  idx.assign(num_slots(p), kEssBit);
  co.assign(r.curl_orients ? num_slots(p) : 0, 0u);
  for (int e = 0; e < p.ne; e++) {
    for (int d = 0; d < P; d++) {
      const int32_t off = r.offsets[(size_t)e * P + d];
      PA_DENSE_REQUIRE(off >= 0 && off < r.lsize, "restriction offset out of range");
      const size_t pos = block_pos(false, KP, e, d);
      idx[pos] = (r.orients && r.orients[(size_t)e * P + d]) ? -1 - off : off;
      if (r.curl_orients) {
        const int8_t *t = r.curl_orients + 3 * ((size_t)e * P + d);
        const int8_t up = d > 0 ? t[-3 + 2] : 0, dn = d + 1 < P ? t[3 + 0] : 0;  // T[d-1][d], T[d+1][d]
        // MFEM's ND face transformations only contain -1, 0, 1 (the reference stores them as int8,
        // restriction.cpp:318-336); two bits per entry
        for (int8_t v : {t[0], t[1], t[2]}) PA_DENSE_REQUIRE(v >= -1 && v <= 1, "curl-orientation entries must be -1, 0 or 1");
        co[pos] = (uint16_t)((t[0] & 3) | ((t[1] & 3) << 2) | ((t[2] & 3) << 4) | ((up & 3) << 6) | ((dn & 3) << 8));
      }
    }
  }
  co2.assign(co.size() / 2, 0u);
  if (co.empty()) return;
  for (size_t b = 0; b < (size_t)p.nb; b++)
    for (int s2 = 0; s2 < KP / 2; s2++)
      for (int l = 0; l < 64; l++)
        co2[(b * (KP / 2) + s2) * 64 + l] = (uint32_t)co[(b * KP + 2 * s2) * 64 + l] | ((uint32_t)co[(b * KP + 2 * s2 + 1) * 64 + l] << 16);
}

// transpose map for the gather form of E^T (counting sort by dof, element order preserved): the copies of dof d are
// ted[tptr[d] .. tptr[d + 1]), each e * P + local dof
inline void build_transpose(const DensePlan &p, const pa_restriction_desc &r, std::vector<int32_t> &tptr, std::vector<int32_t> &ted) {
  const size_t n = (size_t)p.ne * p.P;
  tptr.assign((size_t)r.lsize + 1, 0), ted.resize(n);
  for (size_t k = 0; k < n; k++) tptr[(size_t)r.offsets[k] + 1]++;
  for (int d = 0; d < r.lsize; d++) tptr[d + 1] += tptr[d];
  std::vector<int32_t> fill(tptr.begin(), tptr.end() - 1);
  for (size_t k = 0; k < n; k++) ted[fill[r.offsets[k]]++] = (int32_t)k;
}
// ... and their signed positions in the E-vector of either layout
inline void build_tent(const DensePlan &p, const pa_restriction_desc &r, const std::vector<int32_t> &ted, bool rows,
                       std::vector<int32_t> &tent) {
  tent.resize(ted.size());
  for (size_t k = 0; k < ted.size(); k++) {
    const int32_t pos = (int32_t)block_pos(rows, p.KP, ted[k] / p.P, ted[k] % p.P);
    tent[k] = (r.orients && r.orients[ted[k]]) ? -1 - pos : pos;
  }
}
inline std::vector<int32_t> touched_rows(const std::vector<int32_t> &tptr) {
  std::vector<int32_t> rows;
  for (size_t d = 0; d + 1 < tptr.size(); d++)
    if (tptr[d + 1] > tptr[d]) rows.push_back((int32_t)d);
  return rows;
}

// ---- B: the tables in the kernels' layouts ---------------------------------------------------------------------------------------
struct Tables {
  const double *interp, *deriv;  // [nci Q][P], [ncd Q][P]
  ModeComps m;
  int P, Q;
  double at(int c, int q, int p) const {  // component c of the mode at point q, dof p; zero outside P x Q
    if (q >= Q || p >= P) return 0.0;
    return c < m.nci ? interp[((size_t)c * Q + q) * P + p] : deriv[((size_t)(c - m.nci) * Q + q) * P + p];
  }
};
// The tile row order the kernels rely on: chunks of 16 points, in a chunk the fields, in a field 16 nc rows ordered (point group,
// component) so that a lane ends up with all components of its points.  fn(chunk, nc, cb) once per (chunk, field), in that order.
template <class F>
void walk_fields(const DensePlan &p, ModeComps m, F &&fn) {
  for (int c = 0; c < p.nch; c++)
    for (int f = 0; f < m.nf(); f++) fn(c, m.nc(f), m.cb(f));
}
// MFMA A-operand fragments of the staged kernel, 64 consecutive doubles each: forward [chunk][field][slot s][tile t][lane],
// transposed [chunk][field][row group pi][dof tile pt][lane]
inline void build_fragments(const DensePlan &p, const Tables &T, std::vector<double> &Tf, std::vector<double> &Tt) {
  const int nct = T.m.nct();
  Tf.resize((size_t)p.nch * p.KP * nct * 64), Tt.resize((size_t)p.nch * 4 * nct * p.PT * 64);
  size_t of = 0, ot = 0;
  walk_fields(p, T.m, [&](int c, int nc, int cb) {
    for (int s = 0; s < p.KP; s++)
      for (int t = 0; t < nc; t++)
        for (int lane = 0; lane < 64; lane++) {
          const int i = lane & 15, kq = lane >> 4;
          const int pi = 4 * t + (i >> 2), gl = pi / nc, k = pi % nc;
          Tf[of++] = T.at(cb + k, 16 * c + 4 * gl + (i & 3), 4 * s + kq);
        }
    for (int pi = 0; pi < 4 * nc; pi++)
      for (int pt = 0; pt < p.PT; pt++)
        for (int lane = 0; lane < 64; lane++) {
          const int i = lane & 15, kq = lane >> 4;
          const int gl = pi / nc, k = pi % nc;
          Tt[ot++] = T.at(cb + k, 16 * c + 4 * gl + kq, 16 * pt + i);
        }
  });
}
// resident form: one copy [rows][S], rows in tile order, serves both products
inline void build_resident(const DensePlan &p, const Tables &T, std::vector<double> &L) {
  const int nct = T.m.nct();
  L.assign((size_t)p.rows * p.S, 0.0);
  walk_fields(p, T.m, [&](int c, int nc, int cb) {
    for (int row = 0; row < 16 * nc; row++) {
      const int pi = row >> 2, kqp = row & 3, gl = pi / nc, k = pi % nc;
      for (int d = 0; d < p.P; d++) L[((size_t)(c * nct + cb) * 16 + row) * p.S + d] = T.at(cb + k, 16 * c + 4 * gl + kqp, d);
    }
  });
}
// position-weighted checksum of a table (two sub-operators on "the same basis" are compared through them)
inline double table_checksum(const double *t, size_t n) {
  double c = 0.0;
  if (t)
    for (size_t i = 0; i < n; i++) c += t[i] * (double)(1 + i % 1021);
  return c;
}

}  // namespace densehost
}  // namespace pa
