// Internal declarations shared by the HIP translation units of libpalace_amd.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/palace_amd.h"
#include "pa_devbuf.hpp"
#include "pa_stream_host.hpp"  // kEssBit, kExclBit

struct pa_op;
typedef struct pa_op pa_op_fwd;

// CSR of a fully assembled local operator (pa_op_full_assemble), device arrays
struct pa_csr {
  bool symmetric = true;  // assembled from a symmetric operator (CsrOperator::MultTranspose relies on it)
  int32_t nrows = 0;
  int32_t ncols = 0;  // 0: square
  int64_t nnz = 0;
  pa::DevBuf<int32_t> d_rowptr, d_col;
  pa::DevBuf<double> d_val;
};

namespace pa {

void set_error(const std::string &msg);

struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define PA_HIP(expr)                                                                         \
  do {                                                                                       \
    hipError_t err__ = (expr);                                                               \
    if (err__ != hipSuccess)                                                                 \
      throw pa::Error(std::string(#expr) + " failed: " + hipGetErrorString(err__) + " (" +   \
                      __FILE__ + ":" + std::to_string(__LINE__) + ")");                      \
  } while (0)

#define PA_REQUIRE(cond, msg)                                                   \
  do {                                                                          \
    if (!(cond)) throw pa::Error(std::string(msg) + " [" #cond "]");            \
  } while (0)

// Every C entry point is wrapped: no exception crosses the ABI.
template <typename F>
int guarded(F &&f) {
  try {
    f();
    return 0;
  } catch (const std::exception &e) {
    set_error(e.what());
    return 1;
  } catch (...) {
    set_error("unknown error");
    return 1;
  }
}

template <typename T>
DevBuf<T> dev_upload(const T *host, size_t n, hipStream_t s = nullptr) {
  DevBuf<T> p = dev_alloc<T>(n);
  if (n) PA_HIP(hipMemcpyAsync(p, host, n * sizeof(T), hipMemcpyHostToDevice, s));
  PA_HIP(hipStreamSynchronize(s));
  return p;
}

constexpr int kExclBit16 = 1 << 15;  // flag in the slot permutation: this entry is the only copy of its dof
constexpr int kMaxP1 = 6;  // closed nodes p+1 <= 7
constexpr int kMaxQ1 = 7;

// Packed symmetric pointwise operators (pre-assembled D): double[ne][ncomp][Q], the six upper
// entries of  w detJ adj^T C adj  (mass part, if any) followed by the six of  w detJ Jl^T C Jl
// (curl-curl part, if any).  Shared between an operator and its p-coarsened copies.
struct QData {
  DevBuf<double> d;
  int ncomp = 0;
  int refcount = 0;  // one per Ref<QData>
  // metric form (isotropic coefficients): H = (w / |detJ|) J^T J (six entries) and |detJ| / w per point, a
  // property of the mesh alone, shared by every operator and p-level on it.  Both pointwise operators follow
  // from it in registers:  (w / detJ) J^T c J = c H,   w detJ adj^T c adj = c (|detJ| / w) adj(H).
  bool metric = false;
  // Affine elements (round 6; four points per direction, the streaming H(curl) kernel): an element whose Jacobian is constant has
  // D(q) = w_q D_e -- 6 | 7 | 12 numbers per element instead of per point.  d_aff [ne padded to 4][2 ncomp] pairs of doubles: row
  // 2 c + h of element e = r_c {wz(2h), wz(2h + 1)} with r_c the point-independent factor of component c and wz the 1-D weight
  // along the lane's column (metric component 6, |detJ| / w: g {1 / wz(2h), 1 / wz(2h + 1)}); the kernel multiplies the result of
  // the D stage by the in-plane weight w(ta) w(tb).  batch_aff[b] != 0: the four elements of batch b are all affine (the
  // streaming kernel then reads 4 x 2 ncomp x 16 B instead of 4 x ncomp x 512 B).  The per-point data stays in place: every
  // other consumer (one-shot kernels, diagonal, assembly, the complex forms) is unaffected.  Built once per QData by
  // stream_affine_setup (pa_nd_hex_stream.hip) -- coarsened operators share it with the q-data.
  DevBuf<double> d_aff;
  std::vector<unsigned char> batch_aff;
  bool aff_done = false;
  int n_aff_elems = 0, n_aff_batch_elems = 0;  // affine elements found / of them in all-affine batches (compressed)
  double wq2[2] = {0.0, 0.0};                  // the two distinct 1-D weights (symmetric four-point rule)
  // Column-separable elements (extruded along the local zeta axis: x, y independent of zeta, z linear in it): every component
  // factors as D_c(ta, tb, qz) = wz(qz) r_c(ta, tb) (metric component 6: r / wz(qz)), and lane (ta, tb) of the streaming kernel
  // owns exactly the column qz = 0..3 -- one number per component and lane instead of four.  d_col [ne padded to 4][ncomp][16]
  // doubles (+ 8 of padding: the kernel's second request of a component reads 64 bytes further, unused): r_c(t), the mean over
  // the column of D_c / wz (component 6: of D_6 wz); the kernel multiplies it by wz(qz) (component 6: by 1 / wz(qz)) in registers
  // ahead of its D stage.  batch_col[b] != 0: the four elements of batch b are all column-separable
  // and the batch is not all-affine (those keep the smaller affine rows): 4 x ncomp x 128 B instead of 4 x ncomp x 512 B.
  // Separability along the other two local axes is not looked for.  Built with the affine rows by stream_affine_setup;
  // PALACE_AMD_STREAM_COLUMN=0 switches the form off.  The per-point data stays in place for every other consumer.
  DevBuf<double> d_col;
  std::vector<unsigned char> batch_col;
  int n_col_elems = 0, n_col_batch_elems = 0;  // column-separable elements found (affine ones included) / in column batches
  // every batch of the padded element array is an affine or a column batch: the streaming kernel runs its compact-only form, which
  // never reads `d` (pa_nd_hex_stream.hip: COMPACT; PALACE_AMD_STREAM_COMPACT=0 forces the general form)
  bool all_compact = false;
};

// Geometry factor data (fem/mesh.hpp:27-69): double[ne][11][Q] in HBM.
// Dense (non-tensor) element blocks keep it element-blocked for the MFMA kernel instead:
// double[ceil(ne/16)][11][Qpad][16] (eb == 16).
struct Geom {
  int ne = 0, q1d = 0, Q = 0;
  int eb = 0, Qpad = 0;
  int dim = 3, sdim = 3, nrows = 11;  // 2-D blocks: 6 rows {attr, w detJ, adj(J)^T/detJ (2x2)}; boundary (2 in 3): 8 rows
  DevBuf<double> d_qw;            // quadrature weights (the q_w input of the 2-D curl-curl QFunctions)
  DevBuf<double> d_geom;
  Ref<QData> metric;              // lazily built G = J^T J [ne][6][Q] (tensor hex blocks), see QData
  DevBuf<int32_t> d_attr_e;       // [ne] element attributes (metric form: coefficient lookup in the kernel)
  std::vector<int32_t> h_attr;    // host copy (tensor hex blocks), internal element order
  std::vector<int32_t> eorder;    // internal element p is the caller's element eorder[p] (empty: same order)
  std::vector<double> w1;         // 1-D quadrature weights (tensor hex blocks)
  // geometry from the nodes (hex27 blocks at four points per direction: the streaming curl-curl kernel's GEOMN form, round 5):
  // the 27 x 3 node coordinates of every element in internal element order, [ne padded to 4][27][3], and the 1-D geometry basis
  // at the quadrature points {B [4][3], G [4][3], weights [4]} (device)
  DevBuf<double> d_xnodes, d_gtab;
  std::vector<double> wq;         // quadrature weights (dense blocks), host copy
  int refcount = 1;  // the caller's handle (pa_geom_retain / pa_geom_destroy) and one per Ref<Geom>
  virtual ~Geom() = default;  // (deleted as the pa_geom it was created as)
};

// Parsed coefficient context (coeff_qf.h layout) living in device memory.
struct CoeffDev {
  const int32_t *attr_mat = nullptr;  // [nattr] (device) or nullptr when nattr == 0
  const double *mat = nullptr;        // [nmat * dim*dim] (device), column-major
  int nattr = 0;
};

struct CoeffHost {
  std::vector<int32_t> attr_mat;
  std::vector<double> mat;
  int dim = 3;
  size_t slots = 0;  // number of 8-byte slots this context occupied in the blob
  DevBuf<int32_t> d_attr_mat;
  DevBuf<double> d_mat;
  DevBuf<double> d_mat_t;  // every matrix transposed; only when some matrix is not symmetric
  bool symmetric() const { return !d_mat_t; }
  // the device view the kernels read; inside a TransposeScope (pa_op_mult_transpose: A^T = B^T D(C^T) B for the
  // same trial / test evaluation) the transposed matrices
  CoeffDev dev() const;
};

// RAII switch for the launches of one transposed apply (host side, per thread)
struct TransposeScope {
  TransposeScope(bool on);
  ~TransposeScope();
  static bool active();

private:
  bool prev_;
};

// Offset of component c at point q inside one element's block of packed q-data (H(curl) hexahedra).  In general
// [ncomp][Q]; with 4 points per direction the two points (qz, qz + 1) of a lane's column sit side by side,
// [ncomp][2][16][2], so the element kernels fetch 16 bytes per lane and instruction; with 5 points per direction
// [ncomp][126]: the pairs (qz 0, 1) and (qz 2, 3) of the 25 columns side by side, [2][25][2], then the points qz = 4, [25],
// and one pad entry that keeps every component 16-byte aligned.
__host__ __device__ inline int nd_qd_cstride(int q1d) { return q1d == 5 ? 126 : q1d * q1d * q1d; }
__host__ __device__ inline int nd_qd_offset(int q1d, int c, int q) {
  if (q1d == 4) return ((c * 2 + (q >> 5)) * 16 + (q & 15)) * 2 + ((q >> 4) & 1);
  if (q1d == 5) {
    const int qz = q / 25, t = q - 25 * qz;
    return c * 126 + (qz < 4 ? (qz >> 1) * 50 + 2 * t + (qz & 1) : 100 + t);
  }
  return c * q1d * q1d * q1d + q;
}

// The three forms of a block's streaming tables.  They differ in which entries an element kernel stores straight to y and which
// rows the run gather owns:
//   plain   entries that are the only copy of their dof go straight to y, the gather sums the other dofs
//   masked  the same with the essential dofs read as zero and taken off the direct path: the gather owns their rows too and
//           writes x or 0 there when ParOperator's fix-up is fused (pa_op_set_essential)
//   all     no entry goes straight to y: EVERY dof goes through the E-vector and is owned by the gather, whose epilogue can then
//           consume the sum instead of storing it (the fused smoother step, launch_et_run_gather_step); essential dofs as in masked
enum StreamForm { kStreamPlain = 0, kStreamMasked = 1, kStreamAll = 2 };
inline StreamForm stream_form(bool masked) { return masked ? kStreamMasked : kStreamPlain; }

// What one form owns on the device
struct StreamTables {
  // the words that carry the form's flags, as the block's element kernel reads them: three- and four-point H(curl) the flag
  // words on their own, [ne][16]; five-point H(curl) [ne][ceil(P/64)][32] and H1 [ne][ceil(P/64) + 1][16] the slot words with them
  DevBuf<uint32_t> d_flags;
  DevBuf<uint32_t> d_rchunk;     // [ceil(n_rows / 64)] RunChunk: run-start mask of 64 gathered dofs + run / offset of the first
  DevBuf<int32_t> d_rhdr;        // [n_runs + 1] run headers {first dof | length - 1 | essential, first copy entry}
  DevBuf<int32_t> d_rpos;        // copy positions in d_ye
  int n_rows = 0, n_runs = 0;    // dofs the run gather owns, runs they fall into
  bool ready() const { return d_rhdr != nullptr; }  // the form has been built
};

struct SubOp {
  Ref<Geom> geom;  // (first: the geometry goes after everything that was built on it)
  Ref<QData> qd;  // nullptr: matrix-free D from the geometry data (the reference default)
  int fe_type = 0, p = 0, q1d = 0, P = 0, Q = 0, ne = 0, lsize = 0;
  int qf = 0;
  uint32_t trial_ops = 0, test_ops = 0;
  DevBuf<int32_t> d_lidx;  // [ne][P] signed tensor-order index: >=0 dof, <0 => -(1+dof) flipped
  // sorted order of E / E^T: entry m of element e is its m-th smallest global dof
  DevBuf<int32_t> d_sidx;     // [ne][P] signed sorted index
  DevBuf<int32_t> d_sidx_bc;  // copy with kEssBit on essential dofs (pa_op_set_essential)
  DevBuf<uint16_t> d_perm;    // [ne][P] tensor-order slot of sorted entry m
  // Exclusive dofs (one element copy only, e.g. element interiors): stored straight into y by the
  // element kernel instead of going through the E-vector; the gather kernel then only visits the rest.
  DevBuf<uint16_t> d_perm_x;  // perm with kExclBit16 on exclusive entries (set at finalize)
  DevBuf<int32_t> d_shared;   // list of the dofs the gather kernel still has to sum
  DevBuf<int32_t> d_shared_bc;  // the same with kEssBit on essential dofs (pa_op_set_essential)
  std::vector<int32_t> h_shared;
  int n_shared = 0;
  std::vector<uint16_t> h_perm;
  std::vector<int32_t> h_sidx;   // host copy (needed to build d_sidx_bc)
  // E^T as a gather (default): E-vector scratch and the CSR transpose of lidx
  DevBuf<double> d_ye;      // [ne][P]
  DevBuf<double> d_ye2;     // second E-vector (two right-hand sides), allocated on first use
  DevBuf<int32_t> d_tptr;   // [lsize + 1]
  DevBuf<int32_t> d_tent;   // [ne * P] signed positions into d_ye
  // streaming form (pa_nd_hex_stream.hip): run-compressed index words, byte slots, E^T by runs.  Shared by every form:
  DevBuf<uint32_t> d_idxc;  // [ne][kIdxWords] run-compressed sorted element -> dof index (pa_stream_host.hpp)
  DevBuf<int32_t> d_idxp;   // [ne][16 ceil(P / 16)] the same index word by word (pack_index_plain): four-point H(curl) blocks whose
                            // q-data is all compact (QData::all_compact), read by the compact-only form of the kernel
  bool stream_default = true;  // false: the tables exist for the split-vector apply only, y = A x keeps the one-shot kernel (H1, p < 3)
  std::vector<uint32_t> h_perm_s;  // slot + flag words as pack_index / pack_index_wide lay them out (host; the forms are edited copies)
  // three- and four-point H(curl) kernels: the slot words through a dictionary -- elements whose sorted -> tensor-order permutation
  // agrees share one entry (a structured mesh has a handful: 10 on the 125 440-element bench cylinder), the element's entry
  // number rides in a spare word of its index block
  DevBuf<uint32_t> d_slots;
  int n_slot_patterns = 0;
  DevBuf<double> d_coef_s;    // metric form: [ne][2] scalar mass / curl-curl coefficient per element
  std::vector<char> h_ess_flag;  // the essential flags last fused (stream_set_essential), for stream_build_all
  // ... and per form (StreamForm): plain from build_stream, masked from stream_set_essential, all from stream_build_all
  StreamTables stream[3];
  std::vector<double> Bc, Gc, Bo;  // full 1-D tables [q1d][n] (host)
  DevBuf<double> d_tab;        // the same on the device: [Bo | Bc | Gc]
  bool iso = false;               // every material coefficient is a multiple of the identity
  std::vector<uint8_t> ctx_blob;
  CoeffHost c0, c1;
};

// One sub-operator on a non-tensor element block (pa_dense.hip): dense tables on the FP64 matrix cores.
struct DenseSub {
  Ref<Geom> geom;
  int fe_type = 0, P = 0, Q = 0, Qpad = 0, nch = 0, ne = 0, nb = 0, lsize = 0, KP = 0, PT = 0;
  int qf = 0, mode = 0;
  bool contra = false;  // plane H(div) mass: contravariant map in the vector-mass D (f_apply_hdiv_22)
  bool ye_rows = false;  // E-vector rows by element ([block][element][dof]) instead of by dof (pa_dense.hip: DenseArgs::ye_rows)
  uint32_t trial_ops = 0, test_ops = 0;
  DevBuf<int32_t> d_idx;     // [nb][4 KP][16] signed index (oriented: <0 => -(1+dof) flipped); pads read zero
  DevBuf<int32_t> d_idx_bc;  // copy with kEssBit on essential dofs
  DevBuf<uint8_t> d_ess_flag;  // [lsize] 1 on essential dofs (row fix-up of the split-vector gather)
  DevBuf<uint16_t> d_co;     // [nb][4 KP][16] packed int8 rows / columns of T_e (curl-oriented) or nullptr
  DevBuf<uint32_t> d_co2;    // the same, two dof slots per word: [nb][KP / 2][64] (resident kernel)
  DevBuf<int32_t> d_rows;    // blocks that touch few dofs: the rows they have (sorted), n_rows of them; else nullptr
  int n_rows = 0;
  std::vector<int32_t> h_idx;
  std::vector<int32_t> h_off;  // plain [ne][P] offsets (full assembly)
  DevBuf<double> d_Tf, d_Tt;  // MFMA A-operand fragments of the tables (forward / transposed)
  DevBuf<double> d_L;       // LDS-resident form of the tables (fast path) or nullptr
  DevBuf<double> d_qdata;   // packed pre-assembled D [nb][ncq][Qpad][16] (fast path)
  std::vector<uint16_t> h_co;  // host copy of d_co (restriction compare of the complex form)
  double chk_interp = 0.0, chk_deriv = 0.0;  // checksums of the basis tables (same)
  DevBuf<double> d_ye2;     // second E-vector (imaginary part of the complex form), allocated on first use
  DevBuf<uint8_t> d_affine; // [nb] blocks whose elements all have a constant Jacobian (D_q = (w_q / w_0) D_0) or nullptr
  DevBuf<double> d_wrel;    // [Q4] w_q / w_0
  int n_affine = 0;
  DevBuf<int32_t> d_blist[2];  // mixed meshes: the affine blocks / the others (else nullptr: one kind only)
  int n_blist[2] = {0, 0};
  int L_rows = 0, ncq = 0, num_cu = 0;
  DevBuf<double> d_interp, d_deriv;  // plain tables (diagonal assembly)
  DevBuf<int32_t> d_off;    // plain [ne][P] offsets (diagonal assembly)
  DevBuf<int8_t> d_cor;     // plain curl_orients or nullptr
  DevBuf<double> d_ye;      // E-vector [nb][4 KP][16]
  DevBuf<int32_t> d_tptr, d_tent;
  std::vector<uint8_t> ctx_blob;
  CoeffHost c0, c1;
};

// pa_mixed.hip: one space of a mixed-space operator (plain [ne][P] layouts) and the operator / error integrator itself
struct MixedSide {
  int fe_type = 0, P = 0, lsize = 0, nc = 3;
  std::vector<int32_t> h_off;  // [ne][P] L-vector indices (full assembly)
  DevBuf<int32_t> d_sidx;
  DevBuf<int8_t> d_cor;
  DevBuf<double> d_tabF, d_tabT;
  DevBuf<int32_t> d_tptr, d_tent;
};
struct MixedSub {
  Ref<Geom> geom;
  int ne = 0, Q = 0, qf = 0, kind = 0;
  bool error = false;
  MixedSide s1, s2;  // apply: trial, test; error: first and second input
  CoeffHost c0, c1;
  DevBuf<double> d_ye;
  mutable DevBuf<double> d_ye_t;  // E-vector of the transposed apply (trial side), allocated at its first use
  // sum-factorised form on tensor-product hexahedra (pa_mixed_hex.hip): the two spaces as index-only blocks (sorted signed
  // gather, slot permutation, transpose map and E-vector of each), the 1-D tables shared by both
  std::unique_ptr<SubOp> hex1, hex2;
  DevBuf<int32_t> d_eorder;  // the caller's number of internal element e (error integrator), nullptr: the same order
};

void parse_coeff(const void *blob, size_t bytes, int dim, CoeffHost &out, size_t slot_offset);

// kernels (pa_geom.hip, pa_nd_hex.hip, pa_h1_hex.hip)
void launch_geom(const pa_mesh_desc &mesh, Geom &g, hipStream_t s);
void launch_nd_hex_apply(const SubOp &so, const double *x, double *y, double *ye, bool masked, hipStream_t s,
                         bool accumulate = true, int ess_policy = -1, const double *x1 = nullptr, double *y1 = nullptr,
                         double *ye1 = nullptr);
bool nd_hex_supports_two_rhs(const SubOp &so);
void launch_et_gather2(const SubOp &so, double *y0, double *y1, bool accumulate, hipStream_t s, const double *x0,
                       const double *x1, int ess_policy);
bool nd_hex_fuses_essential(const SubOp &so);
void finalize_exclusive(pa_op_fwd *op);
void launch_et_gather(const SubOp &so, double *y, bool accumulate, hipStream_t s, const double *x = nullptr,
                      int ess_policy = -1);
void launch_nd_hex_qdata(SubOp &so, hipStream_t s);
void launch_nd_hex_metric(SubOp &so, hipStream_t s);
void launch_nd_hex_diag(const SubOp &so, double *diag, hipStream_t s);
// QFunction id of an H(curl) hex block -> its terms and their coefficients (cross 1 / 2: the mixed curl forms)
void nd_terms(const SubOp &so, bool &use_u, bool &use_c, CoeffDev &cm, CoeffDev &cc, int &cross);
// ... of an H1 hex block (mass: values, diffusion: gradient)
void h1_terms(const SubOp &so, bool &use_v, bool &use_g, CoeffDev &cm, CoeffDev &cd);
// pa_nd_hex_q6.hip / pa_h1_hex_q6.hip: six points per direction (PA_HEX_Q6_LIST); launch_nd_hex_apply / launch_h1_hex_apply route here
void launch_nd_hex_q6(const SubOp &so, const double *x, double *y, double *ye, bool masked, hipStream_t s);
void launch_h1_hex_q6(const SubOp &so, const double *x, bool masked, hipStream_t s);
// pa_nd_hex_stream.hip
struct SplitIO;
bool h1_hex_stream_ok(const SubOp &so);       // the streaming form is the default for y = A x
bool h1_hex_stream_capable(const SubOp &so);  // ... its tables can be built (split-vector applies use it at every order)
void launch_h1_hex_stream(const SubOp &so, const double *x, double *y, StreamForm form, hipStream_t s, const SplitIO *split = nullptr);
bool nd_hex_stream_ok(const SubOp &so);
void build_stream(SubOp &so);
void stream_set_essential(SubOp &so, const std::vector<char> &flag);
// Split vectors of a multi-rank apply without L-vector copies: local dofs [0, n_true) are read from x and written to y,
// the ghosts [n_true, lsize) are read from xg0 or xg1 (the parity of the device-resident counter *sel picks the buffer; sel ==
// NULL: xg0) and written to yg (all three unshifted: entry 0 is local dof n_true)
struct SplitIO {
  int n_true;
  const double *xg0, *xg1;
  const unsigned long long *sel;
  double *yg;
};
bool nd_hex_stream_split_ok(const SubOp &so);
// the block's streaming kernel runs its compact-only form (every batch affine or column; PALACE_AMD_STREAM_COMPACT, read per call)
bool nd_hex_stream_compact(const SubOp &so);
// the element kernel of any streaming block on the tables of `form` (H(curl) at three, four or five points; H1 blocks are passed
// on to launch_h1_hex_stream)
void launch_nd_hex_stream(const SubOp &so, const double *x, double *y, StreamForm form, hipStream_t s, const SplitIO *split = nullptr);
// One step of a smoother recurrence consumed inside E^T (round 6): with t = (A x)[d] (the essential rows fixed as in the masked
// apply) the run gather writes  out[d] (+)= x[d] + sd (x[d] - ep[d]) + sr dinv[d] (r0[d] - t)  for every dof and never stores t:
// the Chebyshev step of chebyshev.cpp:204-218 in its accumulated form (linalg.hip: OpChebStep3) without the round trip of A x.
// mode 2, the residual form: with r = r0[d] - t the gather writes  res[d] = r  (if res) and  out[d] = sr dinv[d] r  (if out) --
// r = b - A y of gmg.cpp:186-188 / chebyshev.cpp:196-200 and the first direction d_0 = c_0 D^-1 r of the polynomial.
struct GatherStep {
  double sd, sr;
  const double *dinv, *r0, *ep;  // ep == nullptr: e_{k-1} = 0
  double *out;
  int add;
  double *res;
  int mode;  // 1: Chebyshev step, 2: residual
  // multi-rank (split-vector) form: owned dofs other ranks hold as ghosts (bit 2 of iface_mask[d]) are not finished by this rank's
  // gather -- their sum goes to t_iface[d] and the halo kernel that adds the neighbours' rows applies the step (comm.hip:
  // RestrictAddDirectStep); ghost rows go to the ghost output as in the plain split form.  nullptr: one rank.
  const unsigned char *iface_mask;
  double *t_iface;
  // operators with further (surface) blocks beside the one whose gather runs the step: their contributions, accumulated beforehand,
  // are added to the sum of every row that is not an essential one (nullptr: none).  Dense path only.
  const double *t_add;
};
void launch_et_run_gather2(const SubOp &so, double *y, double *y1, hipStream_t s, const double *x, const double *x1, StreamForm form,
                           int ess_policy, const double *ye1);
bool stream_build_all(SubOp &so);  // the index copies the fused step needs (idempotent; false: this block has no such form)
void launch_nd_hex_stream_all(const SubOp &so, const double *x, hipStream_t s, const SplitIO *split = nullptr);
void launch_et_run_gather_step(const SubOp &so, StreamForm form, const double *x, const GatherStep &step, int ess_policy, hipStream_t s,
                               const SplitIO *split = nullptr);
bool nd_hex_stream5_ok(const SubOp &so);
// pa_nd_hex_stream3.hip: three points per direction (orders 1 and 2), opt-in with PALACE_AMD_STREAM3=1 at operator creation
bool nd_hex_stream3_ok(const SubOp &so);
void launch_nd_hex_stream3(const SubOp &so, const double *x, double *y, StreamForm form, hipStream_t s, const SplitIO *split = nullptr);
void launch_nd_hex_stream5(const SubOp &so, const double *x, double *y, StreamForm form, hipStream_t s, const SplitIO *split = nullptr);
void launch_nd_hex_stream5_complex(const SubOp &sr, const SubOp &si, const double *xr, const double *xi, double *yr, double *yi,
                                   double *ye_i, bool masked, hipStream_t s);
void launch_et_run_gather(const SubOp &so, double *y, bool accumulate, hipStream_t s, const double *x, StreamForm form,
                          int ess_policy, const double *ye = nullptr, const SplitIO *split = nullptr);
void stream_element_coefficients(SubOp &so);
bool nd_hex_stream_complex_ok(const SubOp &sr, const SubOp &si);
void launch_nd_hex_stream_complex(const SubOp &sr, const SubOp &si, const double *xr, const double *xi, double *yr, double *yi,
                                  double *ye_i, bool masked, hipStream_t s);
void launch_h1_hex_apply(const SubOp &so, const double *x, bool masked, hipStream_t s);
void launch_h1_hex_qdata(SubOp &so, hipStream_t s);
void launch_h1_hex_diag(const SubOp &so, double *diag, hipStream_t s);
// pa_rt_hex.hip: Raviart-Thomas hexahedra (mass, div-div, div-div + mass); the E-vector + gather form of E^T only
void launch_rt_hex_apply(const SubOp &so, const double *x, bool masked, hipStream_t s);
void launch_rt_hex_q6(const SubOp &so, const double *x, bool masked, hipStream_t s);  // six points per direction: pa_rt_hex_q6.hip
void launch_rt_hex_qdata(SubOp &so, hipStream_t s);
void launch_rt_hex_diag(const SubOp &so, double *diag, hipStream_t s);
// two right-hand sides per pass (packed D, a compiled pair, PALACE_AMD_TWO_PART != 0): the E-vectors d_ye and d_ye2
bool rt_hex_supports_two_rhs(const SubOp &so);
void launch_rt_hex_apply2(SubOp &so, const double *x0, const double *x1, bool masked, hipStream_t s);
// pa_capi.hip: false when PALACE_AMD_TWO_PART=0 keeps the two-part RT and two-space kernels out (two one-part passes instead)
bool two_part_enabled();

// pa_dense.hip
void launch_geom_dense(const pa_mesh_dense_desc &mesh, Geom &g, hipStream_t s);
std::unique_ptr<DenseSub> make_dense_sub(pa_geom *geom, const pa_restriction_desc &r, const pa_dense_basis_desc &b, int qf,
                         const void *ctx, size_t ctx_size, uint32_t trial_ops, uint32_t test_ops, int height, bool contra = false);
void dense_set_essential(DenseSub &ds, const std::vector<char> &flag);
void launch_dense_apply(const DenseSub &ds, const double *x, bool masked, hipStream_t s, const SplitIO *split = nullptr);
// split: rows >= n_true go to split->yg; ess_policy >= 0 (with split only): essential rows are set to x (1) or 0 (0) here
void launch_dense_gather(const DenseSub &ds, double *y, bool accumulate, hipStream_t s, const double *ye = nullptr,
                         const SplitIO *split = nullptr, const double *x = nullptr, int ess_policy = -1);
bool dense_split_ok(const DenseSub &ds);
// The apply kernel a dense block runs on: resident (tables in LDS) or staged, on curved / affine blocks or on the lists of a mesh
// with both, and 16 PT padded dofs.  The launchers select through it and pa_op_dense_kernel reports it.
enum DenseGeo { kGeoCurved = 0, kGeoAffine = 1, kGeoList = 2 };
struct DenseCell {
  bool resident;
  int geo, PT;
};
DenseCell dense_kernel_cell(const DenseSub &ds);
bool dense_complex_ok(const DenseSub &dr, const DenseSub &di);
void launch_dense_gather_signed(const DenseSub &ds, double *y, double sign, bool skip_ess, hipStream_t s);
// the fused smoother step / residual on a dense block (round 6): the CSR-form gather owns every row; its epilogue consumes the sum
bool dense_fused_step_ok(const DenseSub &ds);
double time_dense_gather(const DenseSub &ds, const int32_t *d_tent);  // ms per launch of the plain E^T gather with this map (set-up)
int dense_gather_group(const DenseSub &ds);
void launch_zero_rows(double *v, const int32_t *rows, int n, hipStream_t s);  // v[rows[i]] = 0
constexpr int kMaxSurfaceBlocks = 8;
struct SurfaceYe {
  const double *ye[kMaxSurfaceBlocks];
};
// out[rows[i]] = sum over the entries of row i (block blk[e], signed position ent[e]) -- the surface blocks of a dense operator in one launch
void launch_surface_rows(const int32_t *rows, int n, const int32_t *row_ptr, const int32_t *ent, const uint8_t *blk, const SurfaceYe &ye,
                         double *out, hipStream_t s);  // lanes per dof of the CSR-form gather (pa_dense.hip: et_gather_group_kernel)
void launch_dense_gather_step(const DenseSub &ds, const double *x, const GatherStep &step, int ess_policy, hipStream_t s,
                              const SplitIO *split = nullptr);
void launch_dense_complex(const DenseSub &dr, const DenseSub &di, const double *xr, const double *xi, double *ye_i, hipStream_t s,
                          bool masked = false);
void launch_dense_diag(const DenseSub &ds, double *diag, hipStream_t s);
void launch_et_gather_raw(int n, const int32_t *tptr, const int32_t *tent, const double *ye, double *y,
                          bool accumulate, hipStream_t s, const int32_t *list = nullptr, const double *x = nullptr,
                          int ess_policy = -1);
// the same for two E-vector / y pairs with one read of the transpose map (the summation order of the one-vector gather)
void launch_et_gather2_raw(int n, const int32_t *tptr, const int32_t *tent, const double *ye0, const double *ye1, double *y0,
                           double *y1, bool accumulate, hipStream_t s, const int32_t *list = nullptr, const double *x0 = nullptr,
                           const double *x1 = nullptr, int ess_policy = -1);

// pa_mixed.hip
std::unique_ptr<MixedSub> make_mixed_sub(pa_geom *geom, const pa_restriction_desc &r1, const pa_dense_basis_desc &b1,
                         const pa_restriction_desc &r2, const pa_dense_basis_desc &b2, int qf, const void *ctx,
                         size_t ctx_size);
std::unique_ptr<MixedSub> make_mixed_gradient_sub(pa_geom *geom, const pa_restriction_desc &r1, const pa_dense_basis_desc &b1,
                                  const pa_restriction_desc &r2, const pa_dense_basis_desc &b2, int comp_stride, int qf,
                                  const void *ctx, size_t ctx_size);
void launch_mixed_apply(const MixedSub &ms, const double *x, double *y, bool accumulate, hipStream_t s, bool transpose = false);
void launch_mixed_error(const MixedSub &ms, const double *u1, const double *u2, double *out, hipStream_t s);
// pa_capi.hip: the tensor-product form of a two-space operator / error integrator; the blocks of its two spaces
std::unique_ptr<MixedSub> make_mixed_hex_sub(pa_geom *geom, const pa_restriction_desc &r1, const pa_basis_desc &b1, const pa_restriction_desc &r2,
                             const pa_basis_desc &b2, int qf, const void *ctx, size_t ctx_size);
// pa_mixed_hex.hip: x1 -> the E-vector of the output block (apply; transpose: hex2 -> hex1) or x1, x2 -> out (error)
void launch_mixed_hex(const MixedSub &ms, const double *x1, const double *x2, double *out, hipStream_t s, bool transpose);
// six points per direction (pa_mixed_hex_q6.hip): so / s2 the input and the other block, kind with the transpose resolved
void launch_mixed_hex_q6(const SubOp &so, const SubOp &s2, const MixedSub &ms, int kind, const double *x1, const double *x2,
                         double *out, hipStream_t s);
// both parts of a complex field in one launch (a compiled pair, PALACE_AMD_TWO_PART != 0)
bool mixed_hex_two_part(const MixedSub &ms);
void launch_mixed_hex2(const MixedSub &ms, const double *x1, const double *x2, const double *x1i, const double *x2i, double *out,
                       hipStream_t s);
// pa_mixed.hip: y0 = A x0, y1 = A x1 / estimates += eta^2(u1, u2) + eta^2(u1i, u2i); one launch where mixed_hex_two_part
void launch_mixed_apply2(const MixedSub &ms, const double *x0, const double *x1, double *y0, double *y1, bool accumulate,
                         hipStream_t s);
void launch_mixed_error2(const MixedSub &ms, const double *u1, const double *u2, const double *u1i, const double *u2i, double *out,
                         hipStream_t s);

}  // namespace pa

struct pa_geom : pa::Geom {};

struct pa_op {
  uint64_t id = 0;  // unique per operator object (pa_op_create / coarsen)
  mutable uint64_t cplx_partner = 0;  // id of the operator the complex-form check below was last made against, and its answer
  mutable int cplx_ok = 0;
  int height = 0, width = 0;
  bool finalized = false;
  bool has_essential = false;
  std::vector<int32_t> ess_sorted;  // the list fused into the index tables (pa_op_set_essential)
  bool symmetric() const;  // every coefficient matrix of every sub-operator is symmetric => A^T = A
  std::vector<std::unique_ptr<pa::SubOp>> subs;
  std::vector<std::unique_ptr<pa::DenseSub>> dsubs;
  std::vector<std::unique_ptr<pa::MixedSub>> msubs;  // trial space != test space (pa_op_add_sub_dense_mixed)
  // fused smoother step of a dense operator with surface blocks (round 6, pa_op_prepare_fused_step): the surface blocks accumulate into
  // t_extra (zero outside their rows; the union of their rows is reset before every use), the volume block's gather adds it
  pa::DevBuf<double> d_t_extra;
  pa::DevBuf<int32_t> d_extra_rows;
  int n_extra_rows = 0;
  // ... by ONE gather over the union of their rows (entries of every surface block, block by block: the order of the accumulating
  // gathers it replaces): row pointers, signed E-vector positions, block numbers
  pa::DevBuf<int32_t> d_urow_ptr, d_uent;
  pa::DevBuf<uint8_t> d_ublk;
};
