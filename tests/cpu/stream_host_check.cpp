// CPU check of the streaming kernel's host-side encodings (palace_amd/csrc/pa_stream_host.hpp): a plain C++ model of
// the decode paths of nd_hex_stream_kernel (E staging, E^T stores) and et_run_gather_kernel is run on random signed
// element->dof maps and compared with the definition  y = E^T D E x  (D = a diagonal per-entry scaling).
// Built and run by tests/test_stream_host.py (g++, no GPU).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <string>

#include "pa_stream_host.hpp"

using namespace pa;
using namespace pa::streamhost;

// A random signed element -> dof map in tensor order and its sorted form as make_sub builds it.  Each element gets P distinct
// dofs, drawn so that entity-like runs of consecutive dofs are shared between elements (blocks of min_block .. min_block + span - 1
// consecutive dofs; mesh entities in a real numbering), random signs.  Small min_block values produce elements with more runs than
// the index block holds, which pack_index has to refuse.
// priv > 0 (the `all` cases) tiles the dof range instead, so that every dof is held and a sizeable share has exactly one copy:
// element e owns the dofs [e w, (e + 1) w), w = stride + priv and P = priv + 2 stride -- `stride` dofs it shares with element
// e - 1, then `priv` dofs nobody else holds -- and holds the shared dofs of element e + 1 (the last one: of element 0) as well;
// lsize = ne w.
struct Map {
  int ne, P, lsize;
  std::vector<int32_t> lidx, sidx, count;
  std::vector<uint16_t> perm;
  std::vector<char> ess;
};
static Map make_map(int ne, int P, int lsize, std::mt19937 &rng, double ess_frac, int min_block, int span, int priv = 0) {
  Map mp{ne, P, lsize, {}, {}, {}, {}, {}};
  mp.lidx.resize((size_t)ne * P);
  for (int e = 0; e < ne; e++) {
    std::vector<char> used(lsize, 0);
    int filled = 0;
    std::vector<int> dofs;
    int tries = 0;
    if (priv > 0) {
      const int stride = (P - priv) / 2, w = stride + priv;
      for (int j = 0; j < w; j++) dofs.push_back(e * w + j);
      for (int j = 0; j < stride; j++) dofs.push_back(((e + 1) % ne) * w + j);
      filled = P;
    }
    while (filled < P) {
      // (after many failed placements -- a nearly full dof range -- fall back to single dofs so the loop always ends)
      const int len = tries > 200 ? 1 : std::min<int>(P - filled, min_block + rng() % span);
      const int d0 = rng() % (lsize - len + 1);
      bool ok = true;
      for (int j = 0; j < len; j++) ok = ok && !used[d0 + j];
      if (!ok) {
        tries++;
        continue;
      }
      for (int j = 0; j < len; j++) used[d0 + j] = 1, dofs.push_back(d0 + j);
      filled += len;
    }
    std::shuffle(dofs.begin(), dofs.end(), rng);
    for (int l = 0; l < P; l++) mp.lidx[(size_t)e * P + l] = (rng() & 1) ? dofs[l] : -1 - dofs[l];
  }
  mp.sidx.resize((size_t)ne * P), mp.perm.resize((size_t)ne * P);
  for (int e = 0; e < ne; e++) {
    std::vector<int> ord(P);
    std::iota(ord.begin(), ord.end(), 0);
    const int32_t *le = &mp.lidx[(size_t)e * P];
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return dof_of(le[a]) < dof_of(le[b]); });
    for (int m = 0; m < P; m++) mp.sidx[(size_t)e * P + m] = le[ord[m]], mp.perm[(size_t)e * P + m] = (uint16_t)ord[m];
  }
  mp.count.assign(lsize, 0);
  for (auto s : mp.sidx) mp.count[dof_of(s)]++;
  mp.ess.assign(lsize, 0);
  for (int d = 0; d < lsize; d++) mp.ess[d] = (rng() % 1000) < ess_frac * 1000;
  return mp;
}

// x, the per-entry scaling D, and the reference: y = E^T D E (x with essential entries zeroed), then y[ess] = x[ess] (DIAG_ONE)
struct Data {
  std::vector<double> x, scale, yref;
};
static Data make_data(const Map &mp, std::mt19937 &rng) {
  Data dt;
  dt.x.resize(mp.lsize), dt.scale.resize((size_t)mp.ne * mp.P);
  std::uniform_real_distribution<double> U(-1, 1);
  for (auto &v : dt.x) v = U(rng);
  for (auto &v : dt.scale) v = U(rng);
  dt.yref.assign(mp.lsize, 0.0);
  for (int e = 0; e < mp.ne; e++)
    for (int l = 0; l < mp.P; l++) {
      const int32_t s = mp.lidx[(size_t)e * mp.P + l];
      const int d = dof_of(s);
      const double u = mp.ess[d] ? 0.0 : (s >= 0 ? dt.x[d] : -dt.x[d]);
      const double v = dt.scale[(size_t)e * mp.P + l] * u;
      dt.yref[d] += s >= 0 ? v : -v;
    }
  for (int d = 0; d < mp.lsize; d++)
    if (mp.ess[d]) dt.yref[d] = dt.x[d];
  return dt;
}

// Model of the 16-lane element kernels (E staging, E^T stores).  The slot words come from the element's block of pp; the flag
// word of lane t of element e is flags[e * fstride + t] -- the last row of that block for the H1 kernel, the array split off by
// split_flag_rows for the three- and four-point H(curl) kernels.  no_direct: the `all` form, where a store to y is an error.
static int elements16(const Map &mp, const std::vector<uint32_t> &ic, const std::vector<uint32_t> &pp, const uint32_t *flags,
                      size_t fstride, int start0, const Data &dt, std::vector<double> &ye, std::vector<double> &y, bool no_direct) {
  const int ne = mp.ne, P = mp.P, nep = (ne + 3) & ~3, npl = (P + 15) / 16, npk = (npl + 3) / 4;
  std::vector<double> sm(P);
  ye.assign((size_t)nep * P, 1e300), y.assign(mp.lsize, 1e300);
  for (int e = 0; e < nep; e++) {
    const uint32_t *row = &pp[(size_t)e * (npk + 1) * 16], *frow = flags + (size_t)e * fstride;
    // E: sorted entries into tensor-order slots (kernel: stage loop)
    std::fill(sm.begin(), sm.end(), 0.0);
    for (int t = 0; t < 16; t++)
      for (int r = 0; r < npl; r++) {
        if (t + 16 * r >= P) continue;
        const unsigned fw = frow[t];
        const int dof = index_dof(&ic[(size_t)e * kIdxWords], t + 16 * r, start0);
        if (dof < 0 || dof >= mp.lsize) return std::printf("decoded dof %d out of range\n", dof), 1;
        const double v = (fw >> (18 + r)) & 1u ? 0.0 : dt.x[dof];
        sm[(row[(r >> 2) * 16 + t] >> (8 * (r & 3))) & 255u] = (fw >> (2 * r)) & 1u ? -v : v;
      }
    // element operator: diagonal scaling in tensor order
    if (e < ne)
      for (int l = 0; l < P; l++) sm[l] *= dt.scale[(size_t)e * P + l];
    // E^T stores
    for (int t = 0; t < 16; t++)
      for (int r = 0; r < npl; r++) {
        if (t + 16 * r >= P) continue;
        const unsigned fl = frow[t] >> (2 * r);
        const double v = sm[(row[(r >> 2) * 16 + t] >> (8 * (r & 3))) & 255u];
        const double sgv = (fl & 1u) ? -v : v;
        if (fl & 2u) {
          const int d = index_dof(&ic[(size_t)e * kIdxWords], t + 16 * r, start0);
          if (no_direct) return std::printf("all form: entry of dof %d on the direct path\n", d), 1;
          if ((frow[t] >> (18 + r)) & 1u) return std::printf("essential dof %d on the direct path\n", d), 1;
          if (e >= ne) return std::printf("pad element %d on the direct path\n", e), 1;
          y[d] = sgv;
        } else {
          ye[(size_t)e * P + t + 16 * r] = sgv;
        }
      }
  }
  return 0;
}

// The same for the wide form (pa_nd_hex_stream5.hip: one element per 32 lanes, 16-bit slot half-words with the flags)
static int elements_wide(const Map &mp, const std::vector<uint32_t> &ic, const std::vector<uint32_t> &pp, const Data &dt,
                         std::vector<double> &ye, std::vector<double> &y, bool no_direct) {
  const int ne = mp.ne, P = mp.P, nep = (ne + 1) & ~1, npl = (P + 31) / 32, npk = (npl + 1) / 2;
  std::vector<double> sm(P);
  ye.assign((size_t)nep * P, 1e300), y.assign(mp.lsize, 1e300);
  auto half = [&](int e, int m) { return (pp[((size_t)e * npk + (m >> 6)) * 32 + (m & 31)] >> (16 * ((m >> 5) & 1))) & 0xffffu; };
  for (int e = 0; e < nep; e++) {
    std::fill(sm.begin(), sm.end(), 0.0);
    for (int m = 0; m < P; m++) {
      const uint32_t h = half(e, m);
      const int dof = index_dof_wide(&ic[(size_t)e * kWideWords], m);
      if (dof < 0 || dof >= mp.lsize) return std::printf("wide: decoded dof %d out of range\n", dof), 1;
      if ((int)(h & kWideSlotMask) >= P) return std::printf("wide: slot out of range\n"), 1;
      const double v = (h & kWideEss) ? 0.0 : dt.x[dof];
      sm[h & kWideSlotMask] = (h & kWideFlip) ? -v : v;
    }
    if (e < ne)
      for (int l = 0; l < P; l++) sm[l] *= dt.scale[(size_t)e * P + l];
    for (int m = 0; m < P; m++) {
      const uint32_t h = half(e, m);
      const double v = sm[h & kWideSlotMask], sgv = (h & kWideFlip) ? -v : v;
      if (h & kWideExcl) {
        if (no_direct) return std::printf("wide all form: an entry on the direct path\n"), 1;
        if (h & kWideEss) return std::printf("wide: essential dof on the direct path\n"), 1;
        if (e >= ne) return std::printf("wide: pad element %d on the direct path\n", e), 1;
        y[index_dof_wide(&ic[(size_t)e * kWideWords], m)] = sgv;
      } else {
        ye[(size_t)e * P + m] = sgv;
      }
    }
  }
  return 0;
}

// The run gather over `rows` (what the gather kernel sees) on the E-vector ye, into y; then y against the reference.
static int gather_and_compare(const char *what, const Map &mp, const std::vector<int32_t> &rows, const Data &dt,
                              const std::vector<double> &ye, std::vector<double> &y) {
  std::vector<uint32_t> code;
  std::vector<RunHdr> hdr;
  std::vector<int32_t> rpos;
  build_runs(mp.ne, mp.P, mp.lsize, mp.sidx.data(), rows, code, hdr, rpos, mp.ess.data());
  // the headers alone name every gathered dof exactly once, with its flag
  size_t k = 0;
  for (size_t r = 0; r + 1 < hdr.size(); r++)
    for (int j = 0; j < run_len(hdr[r]); j++, k++)
      if (k >= rows.size() || run_dof0(hdr[r]) + j != rows[k] || run_ess(hdr[r]) != (mp.ess[rows[k]] != 0))
        return std::printf("%s run headers: run %zu entry %d does not name gathered dof %zu\n", what, r, j, k), 1;
  if (k != rows.size()) return std::printf("%s run headers: %zu of %zu gathered dofs\n", what, k, rows.size()), 1;
  // ... and the chunk masks place every one in its run (the gather's decode: popcount / count-leading-zeros)
  const std::vector<RunChunk> ch = run_chunks(code);
  for (size_t q = 0; q < code.size(); q++) {
    int run, off;
    chunk_decode(ch, q, run, off);
    if (run != (int)((code[q] & 0x7fffffffu) >> 4) || off != (int)(code[q] & 15u))
      return std::printf("%s run chunks: gathered dof %zu decodes to run %d offset %d, code says %u / %u\n", what, q, run, off,
                         (code[q] & 0x7fffffffu) >> 4, code[q] & 15u), 1;
  }
  for (size_t q = 0; q < rows.size(); q++) {
    const int run = (int)((code[q] & 0x7fffffffu) >> 4), j = (int)(code[q] & 15u);
    const int d = run_dof0(hdr[run]) + j;
    if (d != rows[q]) return std::printf("%s run decode: dof %d != %d\n", what, d, rows[q]), 1;
    if (run_ess(hdr[run])) {
      y[d] = dt.x[d];
      continue;
    }
    double s = 0.0;
    for (int p = hdr[run].ptr; p < hdr[run + 1].ptr; p++) s += ye[(size_t)rpos[p] + j];
    y[d] = s;
  }
  double err = 0.0;
  for (int d = 0; d < mp.lsize; d++) err = std::max(err, std::fabs(y[d] - dt.yref[d]));
  const double avg_run = rows.empty() ? 0.0 : (double)rows.size() / (hdr.size() - 1);
  std::printf("%s ne=%d P=%d lsize=%d gathered=%zu runs=%zu (%.2f dofs/run) max err %.3e\n", what, mp.ne, mp.P, mp.lsize, rows.size(),
              hdr.size() - 1, avg_run, err);
  return err < 1e-13 ? 0 : 1;
}

// The masked form and, with_all, the `all` form of one block, built with the functions build_stream, stream_set_essential and
// stream_build_all call (pa_stream_host.hpp) and run through the models above.  pp: the slot + flag words as packed; split: the
// element kernel reads the flag row split off on its own (three- and four-point H(curl)), else inside pp (H1, wide).
static int run_forms(const char *what, const Map &mp, const FlagLayout &fl, bool split, const std::vector<uint32_t> &ic,
                     const std::vector<uint32_t> &pp, int start0, const Data &dt, bool with_all) {
  const bool wide = fl.kind == FlagLayout::kFlagWide;
  const FlagLayout fls{FlagLayout::kFlagSplit, mp.P};
  std::vector<double> ye, y;
  auto elements = [&](const std::vector<uint32_t> &w, bool no_direct) {
    if (wide) return elements_wide(mp, ic, w, dt, ye, y, no_direct);
    if (!split) return elements16(mp, ic, w, w.data() + fl.elem_words() - 16, fl.elem_words(), start0, dt, ye, y, no_direct);
    const std::vector<uint32_t> fw = split_flag_rows(fl, w);
    if (fw.size() != (size_t)fl.padded(mp.ne) * 16) return std::printf("%s: split flag rows of the wrong size\n", what), 1;
    return elements16(mp, ic, w, fw.data(), 16, start0, dt, ye, y, no_direct);
  };
  // masked: essential dofs flagged and off the direct path in the flag words, owned by the run list
  std::vector<uint32_t> pb(pp);
  mark_essential(fl, pb, mp.ne, mp.sidx.data(), mp.ess.data(), true);
  std::vector<int32_t> rows_def;
  for (int d = 0; d < mp.lsize; d++)
    if (mp.count[d] != 1 || mp.ess[d]) rows_def.push_back(d);
  if (gather_rows(mp.ne, mp.P, mp.lsize, mp.sidx.data(), mp.ess.data(), false) != rows_def)
    return std::printf("%s: gather_rows (masked) differs from its definition\n", what), 1;
  if (split) {  // the same edit made on the split rows themselves
    std::vector<uint32_t> fw = split_flag_rows(fl, pp);
    mark_essential(fls, fw, mp.ne, mp.sidx.data(), mp.ess.data(), true);
    if (fw != split_flag_rows(fl, pb)) return std::printf("%s: essential flags differ between the row and the split layout\n", what), 1;
  }
  if (elements(pb, false)) return 1;
  int bad = gather_and_compare(what, mp, rows_def, dt, ye, y);
  if (!with_all) return bad;
  // all: no entry takes the direct path, every dof of [0, lsize) is owned by the run gather, essential rows flagged
  {  // (the case is worth something only if the clear has flags to clear: entries on the direct path that no essential flag takes off it)
    size_t direct = 0;
    for (size_t e = 0; e < (size_t)mp.ne; e++)
      for (int m = 0; m < mp.P; m++)
        if ((pp[fl.word(e, m)] & fl.only_copy(m)) && !mp.ess[dof_of(mp.sidx[e * mp.P + m])]) direct++;
    if (direct * 8 < (size_t)mp.ne * mp.P) return std::printf("%s: only %zu of %zu entries are only copies\n", what, direct, (size_t)mp.ne * mp.P), 1;
  }
  std::vector<uint32_t> pa(pp);
  clear_only_copy(fl, pa);
  mark_essential(fl, pa, mp.ne, mp.sidx.data(), mp.ess.data(), false);
  const std::vector<int32_t> rows_all = gather_rows(mp.ne, mp.P, mp.lsize, mp.sidx.data(), mp.ess.data(), true);
  for (int d = 0; d < mp.lsize; d++)  // (stream_build_all refuses otherwise: the case's parameters are chosen so that this holds)
    if (mp.count[d] == 0) return std::printf("%s: dof %d is held by no element, the all form needs every dof held\n", what, d), 1;
  if ((int)rows_all.size() != mp.lsize) return std::printf("%s: the all form owns %zu of %d dofs\n", what, rows_all.size(), mp.lsize), 1;
  for (int d = 0; d < mp.lsize; d++)
    if (rows_all[d] != d) return std::printf("%s: the all form's row %d is dof %d\n", what, d, rows_all[d]), 1;
  if (split) {
    std::vector<uint32_t> fw = split_flag_rows(fl, pp);
    clear_only_copy(fls, fw);
    mark_essential(fls, fw, mp.ne, mp.sidx.data(), mp.ess.data(), false);
    if (fw != split_flag_rows(fl, pa)) return std::printf("%s: all-form flags differ between the row and the split layout\n", what), 1;
  }
  // (the edit touches flags only: slot words, flip bits and the per-element bits stay)
  for (size_t e = 0; e < (size_t)mp.ne; e++)
    for (int m = 0; m < mp.P; m++) {
      const uint32_t wa = pa[fl.word(e, m)], wp = pp[fl.word(e, m)];
      if ((wa & fl.flipped(m)) != (wp & fl.flipped(m)) || (wa & fl.only_copy(m)))
        return std::printf("%s: all form: flip / only-copy flag of element %zu entry %d\n", what, e, m), 1;
      if (((wa & fl.essential(m)) != 0) != (mp.ess[dof_of(mp.sidx[e * mp.P + m])] != 0))
        return std::printf("%s: all form: essential flag of element %zu entry %d\n", what, e, m), 1;
    }
  for (size_t i = 0; i < pp.size(); i++) {
    const bool flag_word = !wide && (int)(i % fl.elem_words()) >= fl.elem_words() - 16;
    const uint32_t slots = wide ? (kWideSlotMask | kWideSlotMask << 16) : (flag_word ? (kAffBit | kColBit) : ~0u);
    if ((pa[i] & slots) != (pp[i] & slots)) return std::printf("%s: the all form changed word %zu outside its flags\n", what, i), 1;
  }
  const std::string name = std::string(what) + " all";
  if (elements(pa, true)) return 1;
  return bad + gather_and_compare(name.c_str(), mp, rows_all, dt, ye, y);
}

// H(curl) at three / four points (start0 = kIdxStart0: flag words split off) or H1 (kIdxStart0H1: flag row inside the slot block)
static int run_case(int ne, int P, int lsize, unsigned seed, double ess_frac, int min_block = 6, bool expect_ok = true,
                    int start0 = kIdxStart0, int priv = 0) {  // priv > 0: a tiled map (make_map) and the `all` form as well
  std::mt19937 rng(seed);
  const bool with_all = priv > 0;
  const Map mp = make_map(ne, P, lsize, rng, ess_frac, min_block, 12, priv);
  std::vector<uint32_t> ic, pp;
  const bool ok = pack_index(ne, P, lsize, mp.sidx.data(), mp.perm.data(), ic, pp, start0);
  if (ok != expect_ok) return std::printf("pack_index returned %d, expected %d\n", (int)ok, (int)expect_ok), 1;
  if (!ok) return std::printf("ne=%d P=%d: more than %d runs in an element, refused as expected\n", ne, P, kIdxMaxRuns), 0;
  // the compressed index reproduces every entry's dof
  for (int e = 0; e < ne; e++)
    for (int m = 0; m < P; m++)
      if (index_dof(&ic[(size_t)e * kIdxWords], m, start0) != dof_of(mp.sidx[(size_t)e * P + m]))
        return std::printf("index decode: element %d entry %d: %d != %d\n", e, m, index_dof(&ic[(size_t)e * kIdxWords], m, start0),
                           dof_of(mp.sidx[(size_t)e * P + m])), 1;
  const bool h1 = start0 == kIdxStart0H1;
  const FlagLayout fl{FlagLayout::kFlagRow, P};
  if ((size_t)fl.padded(ne) * fl.elem_words() != pp.size()) return std::printf("flag layout: size of the slot words\n"), 1;
  if (!h1) {
    // the per-element bits of build_stream (affine / column batches): on the sixteen flag words of the element, nowhere else, and
    // invisible to the decode below
    const std::vector<uint32_t> before(pp);
    for (size_t e = 0; e < 4 && e < (size_t)fl.padded(ne); e++) set_element_bit(fl, pp, e, kAffBit);
    for (size_t e = 4; e < 8 && e < (size_t)fl.padded(ne); e++) set_element_bit(fl, pp, e, kColBit);
    for (size_t i = 0; i < pp.size(); i++) {
      const size_t e = i / fl.elem_words(), w = i % fl.elem_words();
      const uint32_t want = before[i] | ((int)w >= fl.elem_words() - 16 ? (e < 4 ? kAffBit : (e < 8 ? kColBit : 0u)) : 0u);
      if (pp[i] != want) return std::printf("set_element_bit: word %zu of element %zu\n", w, e), 1;
    }
  }
  const Data dt = make_data(mp, rng);
  return run_forms(h1 ? "h1" : "hcurl", mp, fl, !h1, ic, pp, start0, dt, with_all);
}

// The wide form (pa_nd_hex_stream5.hip: 48-word index block, flags in the slot half-words)
static int run_case_wide(int ne, int P, int lsize, unsigned seed, double ess_frac, int min_block = 6, bool expect_ok = true,
                         int priv = 0) {
  std::mt19937 rng(seed);
  const bool with_all = priv > 0;
  const Map mp = make_map(ne, P, lsize, rng, ess_frac, min_block, 24, priv);
  std::vector<uint32_t> ic, pp;
  const bool ok = pack_index_wide(ne, P, lsize, mp.sidx.data(), mp.perm.data(), ic, pp);
  if (ok != expect_ok) return std::printf("pack_index_wide returned %d, expected %d\n", (int)ok, (int)expect_ok), 1;
  if (!ok) return std::printf("wide ne=%d P=%d: more than %d runs in an element, refused as expected\n", ne, P, kWideMaxRuns), 0;
  for (int e = 0; e < ne; e++)
    for (int m = 0; m < P; m++)
      if (index_dof_wide(&ic[(size_t)e * kWideWords], m) != dof_of(mp.sidx[(size_t)e * P + m]))
        return std::printf("wide index decode: element %d entry %d\n", e, m), 1;
  const FlagLayout fl{FlagLayout::kFlagWide, P};
  if ((size_t)fl.padded(ne) * fl.elem_words() != pp.size()) return std::printf("wide flag layout: size of the slot words\n"), 1;
  const Data dt = make_data(mp, rng);
  return run_forms("wide", mp, fl, false, ic, pp, 0, dt, with_all);
}

// ---- dense path: build_runs_dense against the CSR form of the transpose map -------------------------------------------------------
// Elements of P local dofs made of "entities" of 1 .. 6 consecutive global dofs, each placed at consecutive local positions forwards
// or backwards (an edge seen against its orientation), signs per (element, entity) or -- per_dof_signs -- per entry (runs then break
// inside an entity).  The run form (chunk masks + headers + one position per run and copy) must give exactly the sums of the CSR form.
static int run_case_dense(int ne, int P, int KP, int nent, unsigned seed, bool per_dof_signs) {
  std::mt19937 rng(seed);
  std::vector<int> ent_first, ent_len;
  int lsize = 0;
  for (int k = 0; k < nent; k++) {
    const int len = 1 + (int)(rng() % 6);
    ent_first.push_back(lsize), ent_len.push_back(len), lsize += len;
  }
  lsize += 3;  // a few dofs no element touches (rows the gather writes as zero)
  std::vector<int32_t> offsets((size_t)ne * P);
  std::vector<uint8_t> orients((size_t)ne * P, 0);
  for (int e = 0; e < ne; e++) {
    std::vector<int> order(nent);
    std::iota(order.begin(), order.end(), 0);
    std::shuffle(order.begin(), order.end(), rng);
    int l = 0;
    for (int q = 0; q < nent && l < P; q++) {
      const int k = order[q], len = std::min(ent_len[k], P - l);
      const bool back = rng() & 1u, neg = rng() & 1u;
      for (int i = 0; i < len; i++) {
        offsets[(size_t)e * P + l + i] = ent_first[k] + (back ? len - 1 - i : i);
        orients[(size_t)e * P + l + i] = per_dof_signs ? (uint8_t)(rng() & 1u) : (uint8_t)neg;
      }
      l += len;
    }
    if (l < P) return std::printf("dense case: not enough entities to fill an element\n"), 1;
  }
  const int nb = (ne + 15) / 16;
  std::vector<double> ye((size_t)nb * 4 * KP * 16);
  std::uniform_real_distribution<double> U(-1, 1);
  for (auto &v : ye) v = U(rng);
  auto position = [&](int e, int l) { return ((size_t)(e / 16) * 4 * KP + l) * 16 + (size_t)(e % 16); };
  std::vector<double> yref(lsize, 0.0);
  for (int d = 0; d < lsize; d++) {  // CSR form: copies in element order
    double sum = 0.0;
    for (int e = 0; e < ne; e++)
      for (int l = 0; l < P; l++)
        if (offsets[(size_t)e * P + l] == d) {
          const double v = ye[position(e, l)];
          sum += orients[(size_t)e * P + l] ? -v : v;
        }
    yref[d] = sum;
  }
  std::vector<uint32_t> code, rpos;
  std::vector<RunHdr> hdr;
  build_runs_dense(ne, P, KP, lsize, offsets.data(), orients.data(), code, hdr, rpos);
  const std::vector<RunChunk> ch = run_chunks(code);
  size_t ncopies = 0;
  for (int d = 0; d < lsize; d++) {
    int run, j;
    chunk_decode(ch, (size_t)d, run, j);
    if (run_dof0(hdr[run]) + j != d || j >= run_len(hdr[run])) return std::printf("dense runs: dof %d decodes to run %d offset %d\n", d, run, j), 1;
    double sum = 0.0;
    for (int p = hdr[run].ptr; p < hdr[run + 1].ptr; p++) {
      const uint32_t r = rpos[p];
      const long long at = (long long)(r & kDenseRunPosMask) + ((r & kDenseRunBack) ? -16 * j : 16 * j);
      const double v = ye[(size_t)at];
      sum += (r & kDenseRunNeg) ? -v : v;
    }
    if (sum != yref[d]) return std::printf("dense runs: dof %d: %.17g != %.17g\n", d, sum, yref[d]), 1;
    ncopies += (size_t)(hdr[run + 1].ptr - hdr[run].ptr);
  }
  std::printf("dense ne=%d P=%d lsize=%d runs=%zu positions=%zu (CSR entries %zu) exact\n", ne, P, lsize, hdr.size() - 1, rpos.size(),
              (size_t)ne * P);
  return 0;
}

int main() {
  int bad = 0;
  bad += run_case(37, 144, 2000, 1, 0.05);
  bad += run_case(8, 54, 300, 2, 0.1);
  bad += run_case(5, 12, 40, 3, 0.2);
  bad += run_case(1, 144, 400, 4, 0.0);
  bad += run_case(130, 144, 6000, 5, 0.02);
  bad += run_case(9, 144, 3000, 6, 0.05, 1, false);  // blocks of 1 .. 12 dofs: ~22 runs per element, over the capacity
  bad += run_case(40, 64, 900, 7, 0.05, 1, true, kIdxStart0H1);  // H1 layout: 4 slice words, up to 28 runs
  bad += run_case(11, 27, 300, 8, 0.1, 1, true, kIdxStart0H1);
  bad += run_case_wide(23, 300, 5000, 11, 0.05, 12);  // p = 4
  bad += run_case_wide(7, 144, 1200, 12, 0.1);         // p = 3 on five points
  bad += run_case_wide(6, 54, 400, 13, 0.1);
  bad += run_case_wide(5, 12, 60, 14, 0.2, 1);
  bad += run_case_wide(1, 300, 900, 15, 0.0, 12);
  bad += run_case_wide(4, 300, 6000, 16, 0.05, 1, false);  // short blocks: more than 24 runs, refused
  // the `all` form of every layout on tiled maps (lsize = ne (P + priv) / 2): every dof is held, priv of an element's P entries
  // are only copies (both checked in run_forms)
  bad += run_case(30, 144, 30 * 94, 31, 0.05, 6, true, kIdxStart0, 44);
  bad += run_case(9, 54, 9 * 34, 32, 0.1, 6, true, kIdxStart0, 14);  // nine elements: a batch and a padded one
  bad += run_case(40, 64, 40 * 44, 33, 0.05, 4, true, kIdxStart0H1, 24);
  bad += run_case(9, 27, 9 * 17, 34, 0.1, 4, true, kIdxStart0H1, 7);
  bad += run_case_wide(15, 300, 15 * 190, 35, 0.05, 12, true, 80);  // p = 4
  bad += run_case_wide(9, 54, 9 * 34, 36, 0.1, 6, true, 14);
  bad += run_case_dense(40, 45, 12, 60, 21, false);  // order-3 Nedelec tetrahedron: P = 45, KP = 12
  bad += run_case_dense(33, 20, 8, 25, 22, false);
  bad += run_case_dense(19, 45, 12, 40, 23, true);   // signs per entry: runs break inside the entities
  bad += run_case_dense(1, 10, 4, 6, 24, false);
  return bad;
}

// C entry for tests/test_stream_host.py: statistics of the run form on a real element -> dof map
// (lidx: signed tensor-order index [ne][P] as pa_capi.hip builds it).  Returns the number of runs, -1 on error.
extern "C" int stream_host_run_stats(int ne, int P, int lsize, const int32_t *lidx, int *n_shared, int *n_copies) {
  try {
    std::vector<int32_t> sidx((size_t)ne * P);
    for (int e = 0; e < ne; e++) {
      std::vector<int> ord(P);
      std::iota(ord.begin(), ord.end(), 0);
      const int32_t *le = &lidx[(size_t)e * P];
      std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return dof_of(le[a]) < dof_of(le[b]); });
      for (int m = 0; m < P; m++) sidx[(size_t)e * P + m] = le[ord[m]];
    }
    std::vector<int32_t> count(lsize, 0);
    for (auto s : sidx) count[dof_of(s)]++;
    std::vector<int32_t> shared;
    for (int d = 0; d < lsize; d++)
      if (count[d] != 1) shared.push_back(d);
    std::vector<uint32_t> code;
    std::vector<RunHdr> hdr;
    std::vector<int32_t> rpos;
    build_runs(ne, P, lsize, sidx.data(), shared, code, hdr, rpos);
    *n_shared = (int)shared.size();
    *n_copies = (int)rpos.size();
    return (int)hdr.size() - 1;
  } catch (...) {
    return -1;
  }
}
