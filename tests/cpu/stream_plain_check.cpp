// The plain element -> dof index of the compact-only streaming H(curl) kernels (pa_stream_host.hpp: pack_index_plain) against
// the run-compressed one and the sorted index it is packed from.  Stand-alone: built with -fsanitize=address,undefined by
// tests/test_stream_plain_host.py.  For every entry: index_dof_plain == index_dof == dof_of(sidx), the word's sign == the flip
// bit pack_index puts in the flag word; the pad entries of a partial last slice and the pad elements hold dof 0, unflipped.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "pa_stream_host.hpp"

using namespace pa;
using namespace pa::streamhost;

static int fails = 0;
#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      if (fails++ < 20) {             \
        std::printf("FAIL %s: ", #c); \
        std::printf(__VA_ARGS__);     \
        std::printf("\n");            \
      }                               \
    }                                 \
  } while (0)

// ne elements of P sorted signed entries over lsize dofs: runs of random length (1 .. 16, at most kIdxMaxRuns per element, so that
// pack_index accepts the block), random flips; element 0 starts at dof 0 and holds it flipped (the word -1)
static void make_index(int ne, int P, int lsize, std::mt19937 &rng, std::vector<int32_t> &sidx, std::vector<uint16_t> &perm) {
  sidx.assign((size_t)ne * P, 0);
  perm.assign((size_t)ne * P, 0);
  for (int e = 0; e < ne; e++) {
    // run lengths that sum to P
    std::vector<int> len;
    for (int left = P; left > 0;) {
      const int runs_left = kIdxMaxRuns - (int)len.size();
      int l = std::min(left, 1 + (int)(rng() % 16));
      if (runs_left == 1) l = left;  // (the last run the block can hold takes the rest)
      len.push_back(l);
      left -= l;
    }
    // increasing starts with a gap of at least one dof between runs (so that consecutive runs do not merge)
    const int gaps = lsize - P - (int)len.size();
    int d = (e == 0) ? 0 : (int)(rng() % (unsigned)std::max(1, gaps / 2));
    int m = 0;
    std::vector<int> slot(P);
    for (int i = 0; i < P; i++) slot[i] = i;
    std::shuffle(slot.begin(), slot.end(), rng);
    for (size_t k = 0; k < len.size(); k++) {
      for (int j = 0; j < len[k]; j++, m++, d++) {
        const bool flip = (e == 0 && m == 0) ? true : (rng() & 1u);
        sidx[(size_t)e * P + m] = flip ? -1 - d : d;
        perm[(size_t)e * P + m] = (uint16_t)slot[m];
      }
      d += 1 + (int)(rng() % 3);
    }
    CHECK(d <= lsize, "element %d ran past lsize (%d > %d)", e, d, lsize);
  }
}

static void check_case(int ne, int P, unsigned seed) {
  std::mt19937 rng(seed);
  const int lsize = P + 3 * kIdxMaxRuns + 64;
  std::vector<int32_t> sidx;
  std::vector<uint16_t> perm;
  make_index(ne, P, lsize, rng, sidx, perm);
  CHECK(sidx[0] == -1, "dof 0 flipped is the word -1, got %d", sidx[0]);
  std::vector<uint32_t> ic, pp;
  const bool ok = pack_index(ne, P, lsize, sidx.data(), perm.data(), ic, pp);
  CHECK(ok, "pack_index refused ne %d P %d", ne, P);
  std::vector<int32_t> ip;
  pack_index_plain(ne, P, sidx.data(), ip);
  const int nep = (ne + 3) & ~3, npl = (P + 15) / 16, row = 16 * npl;
  const FlagLayout fl{FlagLayout::kFlagRow, P};
  CHECK((int)ip.size() == nep * row, "table size %zu, expected %d", ip.size(), nep * row);
  CHECK(fl.padded(ne) == nep && fl.slices() == npl, "layout");
  for (int e = 0; e < nep; e++) {
    const int32_t *r = &ip[(size_t)e * row];
    for (int m = 0; m < row; m++) {
      if (e >= ne || m >= P) {  // pad elements, pad entries of a partial last slice
        CHECK(r[m] == 0 && index_dof_plain(r, m) == 0, "pad word e %d m %d = %d", e, m, r[m]);
        continue;
      }
      const int32_t s = sidx[(size_t)e * P + m];
      const int d = dof_of(s);
      CHECK(r[m] == s, "e %d m %d word %d, sorted index %d", e, m, r[m], s);
      CHECK(index_dof_plain(r, m) == d, "e %d m %d plain dof %d, expected %d", e, m, index_dof_plain(r, m), d);
      CHECK(index_dof(&ic[(size_t)e * kIdxWords], m) == d, "e %d m %d compressed dof %d, expected %d", e, m,
            index_dof(&ic[(size_t)e * kIdxWords], m), d);
      const bool flip_flag = (pp[fl.word((size_t)e, m)] & fl.flipped(m)) != 0;
      CHECK((r[m] < 0) == flip_flag, "e %d m %d sign %d, flip bit %d", e, m, r[m] < 0, (int)flip_flag);
    }
  }
  // the flag words of the pad elements carry no flip either
  for (int e = ne; e < nep; e++)
    for (int m = 0; m < P; m++) CHECK((pp[fl.word((size_t)e, m)] & fl.flipped(m)) == 0, "pad element %d entry %d flagged flipped", e, m);
}

int main() {
  const int Ps[3] = {12, 54, 144};  // p = 1, 2, 3
  const int nes[5] = {1, 2, 3, 4, 9};  // ne = 1, 2, 3 (mod 4), a full batch, more than one batch
  unsigned seed = 1;
  for (int P : Ps)
    for (int ne : nes)
      for (int rep = 0; rep < 4; rep++) check_case(ne, P, seed++);
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("stream_plain_check: all checks passed\n");
  return 0;
}
