// tests/host_emul/part_rows_emul.cpp -- TEST-ONLY: level 1 of the bucket partition with per-chunk count rows
// (nova_amd/csrc/msm_partition.hpp k_count_rows -> k_scan_rows -> k_tiles -> k_place_rows, then the unchanged level 2) run thread
// by thread on the CPU (simt.hpp) against DigitsFn + std::sort -- the checks emul.cpp's partition_check makes of the sequence with
// global atomics: the same multiset of (row | sign) words per bucket, contiguous start / end, total = the non-zero digits, the same
// error word.  rows = 0 runs that older sequence (k_hist_hi -> k_tiles -> k_part_hi) through the same checks.  level2 = 0 stops
// after level 1 and its own checks (below): the layout level 2 reads, the total and the error word.
//
// On top of that: the count matrix and the offset matrix start as garbage (the pipeline does not clear them: every row of every
// chunk must be written), guard words around every array the new kernels write must survive, and the intermediate arrays must have
// the layout level 2 expects -- bin regions 16-entry aligned and fully packed, every entry of a region carrying that bin's key bits.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "simt.hpp"

#include "../../nova_amd/csrc/curves.hpp"
#include "../../nova_amd/csrc/msm_pipeline.hpp"

using namespace nmx;

namespace {

constexpr uint32_t kGuard = 64;
template <class T> struct Guarded {  // kGuard pattern words before and after the payload
  std::vector<T> v;
  size_t n;
  T pat;
  Guarded(size_t n_, T pat_, T fill) : v(n_ + 2 * kGuard, fill), n(n_), pat(pat_) {
    for (uint32_t i = 0; i < kGuard; i++) v[i] = v[kGuard + n + i] = pat;
  }
  T* data() { return v.data() + kGuard; }
  bool intact() const {
    for (uint32_t i = 0; i < kGuard; i++)
      if (v[i] != pat || v[kGuard + n + i] != pat) return false;
    return true;
  }
};

template <class A> void launch_kernel(void (*k)(A), uint32_t grid, uint32_t block, const A& a) {
  if (grid == 0) return;
  simt::launch(grid, block, [&] { k(a); });
}

// identity_every != 0: table rows offset + i with i % identity_every == 1 hold the identity (all-zero words): load() returns false
int part_rows_check(const uint8_t* scalars, size_t n, uint32_t c, uint32_t u64_bits, uint32_t grid_override, uint32_t count_grid,
                    uint32_t stride, uint32_t offset, uint32_t identity_every, uint32_t rows, uint32_t level2) {
  constexpr int SF = F_BN254_FR;
  const uint32_t bits = u64_bits ? u64_bits : (uint32_t)FpParams<SF>::BITS;
  MsmShape sh = make_shape((uint32_t)n, bits, 0, c);  // table mode
  if (stride == 0 || !partition_supported(sh, true)) return -2;
  const size_t total = sh.total;
  PartArgs<SF> pa;
  PartBufs& pb = pa.b;
  pb.ps = make_part_shape(sh, true);
  if (!part_rows_supported(sh, pb.ps, true)) return -2;
  if (grid_override) pb.ps.grid1 = grid_override;
  pb.nbuckets = sh.nbuckets;
  std::vector<uint32_t> start(sh.nbuckets + 1), end(sh.nbuckets + 1), ctr(2048 + 3 * kTabStride + 1 + 2 * (size_t)sh.nbuckets), vals(total + 1),
      keys(total + 1), kvals(total + 1);
  Guarded<uint32_t> ent_val(pb.ps.ent_cap, 0xdeadbeefu, 0u);
  Guarded<uint8_t> ent_lo(pb.ps.ent_cap, 0xa5, 0);
  const uint32_t chunks = part_row_chunks(sh.n, pb.ps.bs1);
  Guarded<uint16_t> row_cnt((size_t)chunks * pb.ps.nhi, 0x5a5a, 0xeeee);     // garbage in: nothing clears the matrices
  Guarded<uint32_t> row_rel((size_t)chunks * pb.ps.nhi, 0x5a5a5a5au, 0xeeeeeeeeu);
  std::vector<uint32_t> bases;
  if (identity_every) {
    bases.assign((size_t)stride * 16, 1u);
    for (size_t i = 0; i < n; i++)
      if (i % identity_every == 1) memset(&bases[(offset + i) * 16], 0, 64);
  }
  uint32_t err = 0, tot = 0;
  DigitSrc<SF> src{(const uint32_t*)scalars, identity_every ? bases.data() : nullptr, &err, sh, 0, u64_bits, stride, offset, nullptr, 0};
  pa.src = src;
  pb.hist_hi = ctr.data();
  pb.cur_hi = ctr.data() + 1024;
  pb.tab = ctr.data() + 2048;
  pb.bucket_cnt = ctr.data() + 2048 + 3 * kTabStride + 1;
  pb.bucket_cur = pb.bucket_cnt + sh.nbuckets;
  pb.ent_val = ent_val.data();
  pb.ent_lo = ent_lo.data();
  pb.start = start.data();
  pb.end = end.data();
  pb.vals = vals.data();
  pb.total_out = &tot;
  pb.single_bin = 0;
  if (rows) {
    pb.row_cnt = row_cnt.data();
    pb.row_rel = row_rel.data();
    pb.row_chunks = chunks;
  }
  auto l1 = [&](auto hist, auto part, auto count, auto place) {
    if (rows) {
      launch_kernel(count, count_grid ? count_grid : pb.ps.grid1, pb.ps.bs1, pa);
      launch_kernel(&k_scan_rows<false>, scan_rows_grid(chunks, pb.ps.nhi), 1024u, pb);
      launch_kernel(&k_tiles<false>, 1u, 1024u, pb);
      launch_kernel(place, pb.ps.grid1, pb.ps.bs1, pa);
    } else {
      launch_kernel(hist, pb.ps.grid1, pb.ps.bs1, pa);
      launch_kernel(&k_tiles<false>, 1u, 1024u, pb);
      launch_kernel(part, pb.ps.grid1, pb.ps.bs1, pa);
    }
  };
  if (c == 17) l1(&k_hist_hi<SF, 17, false>, &k_part_hi<SF, 17, false>, &k_count_rows<SF, 17>, &k_place_rows<SF, 17>);
  else if (c == 16) l1(&k_hist_hi<SF, 16, false>, &k_part_hi<SF, 16, false>, &k_count_rows<SF, 16>, &k_place_rows<SF, 16>);
  else l1(&k_hist_hi<SF, 15, false>, &k_part_hi<SF, 15, false>, &k_count_rows<SF, 15>, &k_place_rows<SF, 15>);
  if (!ent_val.intact() || !ent_lo.intact() || !row_cnt.intact() || !row_rel.intact()) return -8;

  // reference: materialised (key, val) pairs grouped by key
  uint32_t err2 = 0;
  DigitSrc<SF> src2 = src;
  src2.err = &err2;
  DigitsFn<SF> df{src2, keys.data(), kvals.data()};
  for (uint32_t i = 0; i < n; i++) df(i);
  if (err != err2) return -3;
  std::vector<std::vector<uint32_t>> ref(sh.nbuckets);
  size_t nz = 0;
  for (size_t e = 0; e < total; e++)
    if (keys[e] < sh.nbuckets) {
      ref[keys[e]].push_back(kvals[e]);
      nz++;
    }
  if (tot != nz) return -4;

  // what level 2 reads: bin b's region [tab[b], tab[b] + size) of ent_val / ent_lo, 16-entry aligned, packed, holding exactly the
  // bin's entries (value words and low key bits as a multiset)
  {
    const uint32_t* tab = pb.tab;
    for (uint32_t b = 0; b < pb.ps.nhi; b++) {
      const uint32_t size = tab[kTabStride + b + 1] - tab[kTabStride + b];
      if (tab[b] % kBinAlign || tab[b + 1] != tab[b] + ((size + kBinAlign - 1) & ~(kBinAlign - 1))) return -9;
      std::vector<uint64_t> got, want;
      for (uint32_t e = 0; e < size; e++) got.push_back(((uint64_t)ent_lo.data()[tab[b] + e] << 32) | ent_val.data()[tab[b] + e]);
      for (uint32_t lo = 0; lo < pb.ps.nlo; lo++) {
        const uint32_t k = (b << pb.ps.LB) + lo;
        if (k < sh.nbuckets)
          for (uint32_t v : ref[k]) want.push_back(((uint64_t)lo << 32) | v);
      }
      std::sort(got.begin(), got.end());
      std::sort(want.begin(), want.end());
      if (got != want) return -10;
    }
  }
  if (rows) {  // the matrices themselves: counts per chunk and bin, exclusive prefix down the columns, totals in hist_hi
    std::vector<uint32_t> run(pb.ps.nhi, 0), want((size_t)chunks * pb.ps.nhi, 0);
    for (uint32_t w = 0; w < sh.W; w++)
      for (uint32_t i = 0; i < sh.n; i++) {
        const uint32_t k = keys[(size_t)w * sh.n + i];
        if (k < sh.nbuckets) want[(size_t)(i / pb.ps.bs1) * pb.ps.nhi + (k >> pb.ps.LB)]++;
      }
    for (uint32_t q = 0; q < chunks; q++)
      for (uint32_t b = 0; b < pb.ps.nhi; b++) {
        const size_t at = (size_t)q * pb.ps.nhi + b;
        if (row_cnt.data()[at] != want[at] || row_rel.data()[at] != run[b]) return -11;
        run[b] += want[at];
      }
    for (uint32_t b = 0; b < pb.ps.nhi; b++)
      if (pb.hist_hi[b] != run[b]) return -12;
    for (uint32_t b = 0; b < 1024; b++)
      if (pb.cur_hi[b]) return -13;  // no cursor is touched on this path
  }

  if (!level2) return 0;
  // level 2, unchanged, over the tiles that exist (the pipeline launches tiles_cap blocks; those past the last tile return at once,
  // and a fiber per thread of each is most of this helper's run time)
  const uint32_t tiles = pb.tab[2 * kTabStride + pb.ps.nhi];
  if (tiles > pb.ps.tiles_cap) return -14;
  launch_kernel(&k_hist_lo<false>, tiles, kTileThreads, pb);
  launch_kernel(&k_part_lo<false>, tiles, kTileThreads, pb);
  uint32_t run = 0;
  for (uint32_t k = 0; k < sh.nbuckets; k++) {
    if (start[k] != run || end[k] != run + ref[k].size()) return -5;
    std::vector<uint32_t> got(vals.begin() + start[k], vals.begin() + end[k]);
    std::sort(got.begin(), got.end());
    std::sort(ref[k].begin(), ref[k].end());
    if (got != ref[k]) return -6;
    run = end[k];
  }
  if (start[sh.nbuckets] != run || end[sh.nbuckets] != run) return -7;
  return 0;
}

}  // namespace

extern "C" {

int emul_part_rows_check(const uint8_t* scalars, size_t n, uint32_t c, uint32_t u64_bits, uint32_t grid_override, uint32_t count_grid,
                         uint32_t stride, uint32_t offset, uint32_t identity_every, uint32_t rows, uint32_t level2) {
  return part_rows_check(scalars, n, c, u64_bits, grid_override, count_grid, stride, offset, identity_every, rows, level2);
}

// first-level block size of the table-mode shape (the tests size their inputs around it)
uint32_t emul_part_rows_bs1(size_t n, uint32_t c, uint32_t u64_bits) {
  const MsmShape sh = make_shape((uint32_t)n, u64_bits ? u64_bits : (uint32_t)FpParams<F_BN254_FR>::BITS, 0, c);
  PartShape ps;
  if (!make_part_shape(sh, true, &ps) || !part_rows_supported(sh, ps, true)) return 0;
  return ps.bs1;
}

// the whole pipeline with MsmArgs::part_rows through msm_pipeline() is covered on the device (tests/test_gpu_part_rows.py); here the
// default-constructed arguments must leave the rows off, as every backend that predates them expects
uint32_t emul_part_rows_default() { return MsmArgs{}.part_rows; }
}
