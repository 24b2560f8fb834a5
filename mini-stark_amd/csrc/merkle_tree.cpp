// merkle_tree.cpp — MerkleTree::new (merkle.rs:81-177) on the kernel family of the context's digest (msmerkle::with_digest, digest.hpp: SHA-256, BLAKE2s-256, BLAKE3,
// Keccak-256 / SHA3-256): replicated, sharded by leaf-group residue (digest all-to-all) and sharded by contiguous range; ms_merkle_commit.  Also the host side of
// ms_grind (grind.hpp): the other pure-hashing stage that picks its kernel by the context's digest.
#include "ctx.hpp"
#include "digest.hpp"
#include "grind.hpp"

namespace msctx {

// src/merkle.rs:89-118 (shape checks and node count)
template <class F>
int Ctx<F>::tree_shape(size_t leaf_num, size_t lpn, size_t ic, TreeShape* ts) {
  if (lpn == 0 || ic < 2 || !is_pow2(ic)) return fail(MS_ERR_SHAPE, "merkle: bad leafs_per_node / inner_children");
  const size_t node_num = leaf_num / lpn;
  long lg = log_two_k(node_num, ic);
  if (lg < 0) return fail(MS_ERR_SHAPE, lg == -1 ? "number if not a power of 2" : "number if not a power of base");
  if (leaf_num % lpn != 0) return fail(MS_ERR_SHAPE, "merkle: leaf_num % leafs_per_node != 0");
  if (lg >= 64 || node_num == 0) return fail(MS_ERR_SHAPE, "Tree is not full!");
  ts->leaf_num = leaf_num; ts->lpn = lpn; ts->ic = ic; ts->levels = (size_t)lg + 1;
  size_t total = 0, m = node_num;
  for (;;) { total += m; if (m == 1) break; m /= ic; }
  ts->nodes = total; ts->local_nodes = total; ts->Mloc = 0; ts->sharded = false;
  return 0;
}

// leaf-group digests of `ngroups` groups into `out`: LeafHashKernel + the compacted pad-only blocks it deferred
template <class F> template <int EL>
int Ctx<F>::leaf_hash(const T* base, size_t col_stride, size_t row_stride, size_t limb_stride, u32 width, size_t lpn, size_t ngroups, u32* out,
              size_t g_first, u32 run_len, u32 run_stride, const msmerkle::LinColSpec* lin, size_t out_g0) {
  if (ngroups >> 32) return fail(MS_ERR_SHAPE, "more than 2^32 leaf groups");
  const size_t nwg = grid1(ngroups, msmerkle::THREADS);
  // one launch of the leaf kernel LK; counters / cap: the deferred-block lists of a family that has them, or null / 0
  auto launch = [&](auto kernel, u32* counters, size_t cap) -> int {
    typedef decltype(kernel) LK;
    typename LK::Params lp;
    lp.base = base; lp.col_stride = col_stride; lp.row_stride = row_stride; lp.limb_stride = limb_stride;
    lp.width = width; lp.lpn = (u32)lpn; lp.zero_as_empty = zae; lp.ngroups = ngroups; lp.nodes = out;
    lp.ovf_count = counters; lp.ovf = counters ? d_ovf.as<u32>() : nullptr; lp.ovf_cap = (u32)cap;
    lp.g_first = g_first; lp.run_len = run_len; lp.run_stride = run_stride; lp.lin = lin; lp.out_g0 = out_g0;
    next_bytes = (double)ngroups * (lpn * EL * sizeof(T) + 32);
    CK(run<LK>(K_LEAF_HASH, (unsigned)nwg, 1, msmerkle::THREADS, LK::lds_bytes(), lp));
    return 0;
  };
  // the launches of the family DG.  SHA-256 (DG::DEFERS): final blocks without message bytes go to lists and a compacted follow-up kernel.  BLAKE2s-256 / BLAKE3:
  // no such block exists; Keccak-256 / SHA3-256: a block of padding only is absorbed in place - one launch, no lists, no zeroed counters
  auto hash = [&](auto family) -> int {
    typedef decltype(family) DG;
    // deferred pad-only blocks: OVF_LISTS lists, list l fed by the workgroups bx = l (mod OVF_LISTS); capacity = all their threads
    const size_t lists = msmerkle::OVF_LISTS, cap = DG::DEFERS ? ((nwg + lists - 1) / lists) * msmerkle::THREADS : 0;
    void* counters = nullptr;
    if constexpr (DG::DEFERS) {
      if (d_ovf.ensure(lists * cap * msmerkle::OVF_WORDS * 4)) return fail(MS_ERR_NOMEM, "deferred-block lists");
      RQ(zero_alloc(lists * 4, &counters));
    }
    // long messages (wide rows): the buffer of LAZY_BLOCKS blocks that compresses wave-synchronously
    if (lpn * EL >= (size_t)leaf_lazy_min) RQ(launch(msmerkle::LeafHashKernel<F, EL, true, DG>(), reinterpret_cast<u32*>(counters), cap));
    else RQ(launch(msmerkle::LeafHashKernel<F, EL, false, DG>(), reinterpret_cast<u32*>(counters), cap));
    if constexpr (DG::DEFERS) {
      msmerkle::PadOnlyBlockKernel::Params pp{reinterpret_cast<u32*>(counters), d_ovf.as<u32>(), (u32)cap, out};
      const size_t used = nwg < lists ? nwg : lists, per_list = grid1(cap, msmerkle::THREADS);
      CK(run<msmerkle::PadOnlyBlockKernel>(K_LEAF_HASH, (unsigned)used, (unsigned)(per_list < (size_t)msmerkle::PAD_GRID_Y ? per_list : (size_t)msmerkle::PAD_GRID_Y), msmerkle::THREADS, 0, pp));
    }
    return 0;
  };
  return msmerkle::with_digest(digest, [&](auto family) -> int {
    typedef decltype(family) DG;
    if constexpr (std::is_same<DG, msmerkle::Blake3Kernels>::value) {
      // an upper bound of a leaf group's message: every limb at its longest, with its share of the extension's affixes.  Up to one chunk: the kernels without
      // a chunk tree; up to MAX_BYTES: the multi-chunk instances; beyond: refused (never a wrong digest)
      const size_t bound = lpn * EL * (size_t)msmerkle::LeafHashKernel<F, EL, false, DG>::MAX_BYTES;
      if (lpn > DG::MAX_BYTES || bound > DG::MAX_BYTES)
        return fail(MS_ERR_ARG, "BLAKE3: a leaf group's message may exceed 16384 bytes (leafs_per_node x limbs x longest decimal): not supported by the BLAKE3 kernels");
      if (bound > DG::CHUNK_BYTES) return hash(typename DG::Multi());
    }
    return hash(family);
  });
}

template <class F> template <int EL>
int Ctx<F>::tree_build(const T* base, size_t col_stride, size_t row_stride, size_t limb_stride, u32 width, const TreeShape& ts, DevBuf& nodes, const msmerkle::LinColSpec* lin) {
  if (nodes.ensure(ts.nodes * 32)) return fail(MS_ERR_NOMEM, "merkle nodes");
  const size_t ngroups = ts.leaf_num / ts.lpn;
  RQ((leaf_hash<EL>(base, col_stride, row_stride, limb_stride, width, ts.lpn, ngroups, nodes.as<u32>(), 0, 0, 0, lin)));
  RQ(inner_levels(nodes.as<u32>(), ngroups, ts.ic));
  return 0;
}

// `grid` workgroups of the level kernel of the context's digest (ic == 2: the binary tree's instance)
template <class F>
int Ctx<F>::inner_launch(unsigned grid, const msmerkle::InnerHashParams& ip) {
  return msmerkle::with_digest(digest, [&](auto family) -> int {
    typedef decltype(family) DG;
    if constexpr (std::is_same<DG, msmerkle::Blake3Kernels>::value) {
      if (ip.ic > DG::MAX_BYTES / 32) return fail(MS_ERR_ARG, "BLAKE3: inner nodes of more than 512 children (16384 bytes) are not supported by the BLAKE3 kernels");
      if (ip.ic > DG::CHUNK_BYTES / 32) {   // more than one chunk: the chunk tree, chaining values in LDS
        CK(run<typename DG::InnerMulti>(K_INNER_HASH, grid, 1, msmerkle::THREADS, DG::InnerMulti::lds_bytes(), ip));
        return 0;
      }
    }
    if (ip.ic == 2) CK(run<typename DG::Inner2>(K_INNER_HASH, grid, 1, msmerkle::THREADS, 0, ip));
    else CK(run<typename DG::Inner>(K_INNER_HASH, grid, 1, msmerkle::THREADS, 0, ip));
    return 0;
  });
}

template <class F>
int Ctx<F>::inner_levels(u32* nodes, size_t nchildren, size_t ic, bool final_levels, u8* rec_out) {
  size_t child_off = 0;
  // rec_out (a subtree of a sharded tree, final_levels false): the launch that produces the subtree's root also stores the rank's record of the root all-gather -
  // root at rec_out, the aux word (res.shard_word(), if any) 32 bytes behind it - instead of a fill and two copy launches behind the subtree (r05)
  unsigned long long* const shard_aux = res.shard_word();
  bool rec_done = false;
  auto to_rec = [&](msmerkle::InnerHashKernel::Params& ip) {
    ip.host_root = reinterpret_cast<u32*>(rec_out);
    if (shard_aux) { ip.aux_src = shard_aux; ip.aux_dst = reinterpret_cast<unsigned long long*>(rec_out + 32); }
    rec_done = true;
  };
  while (nchildren > 1) {
    msmerkle::InnerHashKernel::Params ip;
    ip.nodes = nodes; ip.child_off = child_off; ip.nchildren = nchildren; ip.ic = (u32)ic; ip.host_root = nullptr; ip.aux_src = nullptr; ip.aux_dst = nullptr; ip.flag = msrt::HostFlag{nullptr, 0};
    const size_t nparents = nchildren / ic;
    if (ic == 2 && nparents <= subtree_parents && (nchildren & (nchildren - 1)) == 0) {   // latency-bound levels: up to 9 of them per launch, children in LDS
      typedef msmerkle::InnerSubtreeKernel SK;
      u32 nl = 0; for (size_t m = nchildren; m > 1 && nl < (u32)SK::MAX_LEVELS; m >>= 1) nl++;
      const size_t left = nchildren >> nl;
      if (final_levels && left == 1) RQ(res.attach(ip));   // (joins the side stream: this launch forwards the length word its scan produces)
      else if (rec_out && left == 1) to_rec(ip);
      ip.nlevels = nl;
      next_bytes = (double)nchildren * 32 * 2;
      CK(msmerkle::with_digest(digest, [&](auto family) { return run_coop<typename decltype(family)::Subtree>(K_INNER_HASH, (unsigned)left, SK::THREADS, SK::lds_bytes(), ip); }));
      for (u32 l = 0; l < nl; l++) { child_off += nchildren; nchildren >>= 1; }
      continue;
    }
    if (final_levels && (nparents == 1 || nparents <= (size_t)tree_top_parents)) RQ(res.attach(ip));   // (the launch below is the tree's last either way: the fused top, or the level whose one parent is the root)
    else if (rec_out && (nparents == 1 || nparents <= (size_t)tree_top_parents)) to_rec(ip);
    if (nparents <= (size_t)tree_top_parents) {  // fused tree top: one workgroup walks the remaining levels
      u32 nl = 0; for (size_t m = nchildren; m > 1; m /= ic) nl++;
      ip.nlevels = nl;
      next_bytes = (double)nchildren * 32 * 2;
      RQ(inner_launch(1, ip));
      break;
    }
    ip.nlevels = 1;
    next_bytes = (double)nparents * (ic * 32 + 32);
    RQ(inner_launch((unsigned)((nparents + msmerkle::THREADS - 1) / msmerkle::THREADS), ip));
    child_off += nchildren; nchildren = nparents;
  }
  if (rec_out && !rec_done) {   // no launch took the record along (a one-digest "subtree"): by copies
    CK(msrt::d2d(rec_out, reinterpret_cast<u8*>(nodes) + (child_off + nchildren - 1) * 32, 32, stream));
    if (shard_aux) CK(msrt::d2d(rec_out + 32, shard_aux, 8, stream)); else CK(msrt::memset_dev(rec_out + 32, 0, 8, stream));
  }
  return 0;
}

// Sharded MerkleTree::new over a binary tree of M = leaf_num/lpn leaf groups, of which this rank hashes the groups
// j = rank + W*i found at local group index i of the view (base, strides): digest all-to-all, subtree, root all-gather, top.
template <class F> template <int EL>
int Ctx<F>::tree_build_sharded(const T* base, size_t col_stride, size_t row_stride, size_t limb_stride, u32 width, TreeShape& ts, DevBuf& nodes, const msmerkle::LinColSpec* lin) {
  const size_t W = (size_t)sh_world, M = ts.leaf_num / ts.lpn, Mloc = M / W, per = Mloc / W;
  if (ts.ic != 2 || per == 0) return fail(MS_ERR_STATE, "sharded tree needs a binary tree with at least world^2 leaf groups");
  if (Mloc * 32 > xcap) return fail(MS_ERR_NOMEM, "exchange buffers too small for the sharded commitment (need 32 * leaf groups / world bytes)");
  const size_t sub_nodes = 2 * Mloc - 1, top_nodes = 2 * W - 1;
  if (nodes.ensure((sub_nodes + top_nodes) * 32)) return fail(MS_ERR_NOMEM, "merkle nodes");
  // The digest all-to-all overlaps the leaf hashing (r03): the local groups are hashed in `S` slices - slice s = the s-th part of EVERY peer's chunk - and
  // the digests of slice s travel (RCCL: on the context's communication stream, ordered by events) while slice s + 1 is hashed.  MS_SHARD_SLICES (4) /
  // MS_SHARD_SLICE_MIN (1024 groups per peer and slice; below that the commitment goes out in one piece).
  const size_t want_slices = (rccl_comm && !shard_slices_set) ? 1 : (size_t)shard_slices;
  const size_t S = (want_slices > 1 && per % want_slices == 0 && per / want_slices >= shard_slice_min) ? want_slices : 1;
  PartScope part(this);
  if (S == 1) {
    RQ((leaf_hash<EL>(base, col_stride, row_stride, limb_stride, width, ts.lpn, Mloc, reinterpret_cast<u32*>(xs), 0, 0, 0, lin)));
    RQ(exchange(MS_XCHG_ALL_TO_ALL, per * 32));
  } else {
    const size_t q = per / S;
    for (size_t sl = 0; sl < S; sl++) {
      RQ((leaf_hash<EL>(base, col_stride, row_stride, limb_stride, width, ts.lpn, W * q, reinterpret_cast<u32*>(xs), sl * q, (u32)q, (u32)per, lin)));
      RQ(exchange_slice(sl * q * 32, per * 32, q * 32, (int)sl, (int)S));
    }
  }
  msmerkle::InterleaveDigestsKernel::Params ik{reinterpret_cast<const msmerkle::uint4_t*>(xr), reinterpret_cast<msmerkle::uint4_t*>(nodes.p), per, (u32)W};
  CK(run<msmerkle::InterleaveDigestsKernel>(K_IO, grid1(Mloc * 2, msmerkle::InterleaveDigestsKernel::THREADS), 1, msmerkle::InterleaveDigestsKernel::THREADS, 0, ik));
  return finish_sharded_tree(ts, nodes, Mloc);
}

template <class F>
int Ctx<F>::finish_sharded_tree(TreeShape& ts, DevBuf& nodes, size_t Mloc) {
  const size_t W = (size_t)sh_world, sub_nodes = 2 * Mloc - 1, top_nodes = 2 * W - 1;
  constexpr size_t REC = msmerkle::ShardTopTreeKernel::REC;
  if (W * REC > xcap) return fail(MS_ERR_NOMEM, "exchange buffers too small for the subtree roots");
  // the subtree; its last launch leaves this rank's record (root | aux word) in the send buffer.  (Bytes 40 .. 64 of a record are never read.)
  { PartScope part(this); RQ(inner_levels(nodes.as<u32>(), Mloc, 2, false, xs)); }
  RQ(exchange(MS_XCHG_ALL_GATHER, REC));
  // the W records -> the top's leaves, the maximum aux word, and the levels above them, in one launch; root (and the length word riding on the commitment) to the host
  u8* top = nodes.as<u8>() + sub_nodes * 32;
  typedef msmerkle::ShardTopTreeKernel TT;
  if (W > ((size_t)1 << msmerkle::InnerSubtreeKernel::MAX_LEVELS)) return fail(MS_ERR_STATE, "sharded tree: more ranks than the top kernel's levels");
  typename TT::Params tk;
  memset(&tk, 0, sizeof tk);
  tk.recs = xr; tk.W = (u32)W; tk.aux_max = res.shard_word();
  tk.tree.nodes = reinterpret_cast<u32*>(top); tk.tree.child_off = 0; tk.tree.nchildren = W; tk.tree.ic = 2;
  u32 tl = 0; while (((size_t)1 << tl) < W) tl++;
  tk.tree.nlevels = tl;
  RQ(res.attach(tk.tree));
  CK(run_coop<TT>(K_INNER_HASH, 1, TT::THREADS, TT::lds_bytes(), tk));
  ts.sharded = true; ts.Mloc = Mloc; ts.local_nodes = sub_nodes + top_nodes;
  return 0;
}

// MerkleTree::new over data EVERY rank holds (the raw trace): rank k hashes the contiguous leaf groups [k*M/W, (k+1)*M/W) - no digest exchange at all -
// builds that subtree, and the ranks all-gather the W subtree roots
template <class F> template <int EL>
int Ctx<F>::tree_build_sharded_contiguous(const T* base, size_t col_stride, size_t row_stride, size_t limb_stride, u32 width, TreeShape& ts, DevBuf& nodes) {
  const size_t W = (size_t)sh_world, M = ts.leaf_num / ts.lpn, Mloc = M / W;
  if (ts.ic != 2 || Mloc == 0 || (Mloc >> 32)) return fail(MS_ERR_STATE, "sharded tree needs a binary tree with at least world leaf groups");
  if (nodes.ensure((2 * Mloc - 1 + 2 * W - 1) * 32)) return fail(MS_ERR_NOMEM, "merkle nodes");
  // group g of the launch is leaf group rank*Mloc + g (one run of Mloc groups); its digest lands at nodes[g] (out_g0 = the rank's first group)
  PartScope part(this);
  RQ((leaf_hash<EL>(base, col_stride, row_stride, limb_stride, width, ts.lpn, Mloc, nodes.as<u32>(), (size_t)sh_rank * Mloc, (u32)Mloc, 0, nullptr, (size_t)sh_rank * Mloc)));
  return finish_sharded_tree(ts, nodes, Mloc);
}

// ------------------------------------------------------------------ standalone entry points
template <class F>
int Ctx<F>::merkle_commit(const u64* leafs, size_t leaf_num, int ext, size_t lpn, size_t ic, u8* nodes_out, size_t cap, size_t* nn, u8* root) {
  if (!leafs && leaf_num) return fail(MS_ERR_ARG, "null leafs");
  if (ext != 1 && ext != E) return fail(MS_ERR_ARG, "ext must be 1 or the field's extension degree");
  TreeShape ts;
  RQ(tree_shape(leaf_num, lpn, ic, &ts));
  if (!canonical(leafs, leaf_num * ext)) return fail(MS_ERR_ARG, "leaf not canonical");
  DevBuf dl, dn;
  if (dl.ensure(leaf_num * ext * sizeof(T))) return fail(MS_ERR_NOMEM, "leafs");
  auto idle = scope_exit([&] { msrt::sync(stream); });   // (before dl and dn go, behind whatever the stage's guard enqueues)
  auto stage = res.expect();
  RQ(upload_narrow(leafs, leaf_num * ext, dl.as<T>()));
  // AoS view: element f limb k at base + f*ext + k
  RQ((ext == 1) ? tree_build<1>(dl.as<T>(), 0, 1, 0, 1, ts, dn) : tree_build<E>(dl.as<T>(), 0, (size_t)ext, 1, 1, ts, dn));
  if (nn) *nn = ts.nodes;
  if (nodes_out) {
    if (cap < ts.nodes) return fail(MS_ERR_ARG, "nodes_out too small");
    CK(msrt::d2h(nodes_out, dn.p, ts.nodes * 32, stream));
    CK(msrt::sync(stream));
  }
  if (root) RQ(read_root(dn, ts, root));
  return MS_OK;
}

// ------------------------------------------------------------------ build-defined: proof-of-work grinding (include/ministark.h; kernel: grind.hpp)
// Launches of at most grind_launch_max nonces in ascending order on the context's stream; the found word (res.word(GRIND): 0, or ~ the smallest hit) comes home
// through the stage results.  The first look follows the first launch (short: sized by `bits`; the usual grind ends there); after that GRIND_AHEAD launches are enqueued per look - a launch
// behind a hit finds the word set at its first read and returns at once.  Field-independent: a sharded context runs it like any other, every rank for itself.
template <class F>
int Ctx<F>::grind(const u8* seed, u32 bits, u64 start, u64 limit, u64* nonce) {
  if (!seed || !nonce) return fail(MS_ERR_ARG, "grind: null argument");
  if (bits > MS_GRIND_MAX_BITS) return fail(MS_ERR_ARG, "grind: more than MS_GRIND_MAX_BITS bits");
  if (limit == 0 || limit > ~(u64)0 - start) return fail(MS_ERR_ARG, "grind: limit must be positive and start + limit at most 2^64 - 1");
  constexpr int GRIND_AHEAD = 4;
  msmerkle::GrindParams gp;
  memcpy(gp.seed, seed, 32);
  gp.mask = bits ? ~(u64)0 << (64 - bits) : 0;
  gp.found = res.word(Results::GRIND);
  int cus = 0;
  if (!grind_grid) CK(msrt::cu_count(device, &cus));
  const u64 end = start + limit;
  u64 at = start;
  for (int ahead = 1; at < end; ahead = GRIND_AHEAD) {
    auto stage = res.expect(gp.found);
    for (int k = 0; k < ahead && at < end; k++) {
      gp.start = at; gp.n = end - at < grind_launch_max ? end - at : grind_launch_max;
      // the first launch covers 64 times the expected distance to a hit (it fails with probability e^-64) and no more: at few bits a whole grid's worth of
      // threads each find a hit of their own in the first sweep (measured at 4 bits: 0.17 ms of kernel time for a search that needs 16 hashes, 0.01 ms this way;
      // DESIGN 3.2)
      if (at == start && bits + 6 < 64 && gp.n > ((u64)1 << (bits + 6))) gp.n = (u64)1 << (bits + 6);
      RQ(msmerkle::with_digest(digest, [&](auto family) -> int {
        typedef msmerkle::GrindPolicy<decltype(family)> GD;
        typedef msmerkle::GrindKernel<decltype(family)> GK;
        const u64 cap = grind_grid ? grind_grid : (u64)cus * GD::WGS_PER_CU, want = (gp.n + GK::THREADS - 1) / GK::THREADS;
        next_bytes = 0;
        CK(run_coop<GK>(K_GRIND, (unsigned)(want < cap ? want : cap), GK::THREADS, 0, gp));
        return 0;
      }));
      at += gp.n;
    }
    unsigned long long word = 0;
    RQ(res.collect(nullptr, nullptr, &word));
    if (word) { *nonce = ~word; return MS_OK; }
  }
  return fail(MS_ERR_OUT_OF_RANGE, "grind: no nonce of the range satisfies the proof of work");
}

// the members this unit defines, for both fields (the other units see declarations only)
#define MS_INSTANTIATE(FF) \
  template int Ctx<FF>::tree_shape(size_t leaf_num, size_t lpn, size_t ic, Ctx<FF>::TreeShape* ts); \
  template int Ctx<FF>::inner_launch(unsigned grid, const msmerkle::InnerHashParams& ip); \
  template int Ctx<FF>::inner_levels(u32* nodes, size_t nchildren, size_t ic, bool final_levels, u8* rec_out); \
  template int Ctx<FF>::finish_sharded_tree(Ctx<FF>::TreeShape& ts, DevBuf& nodes, size_t Mloc); \
  template int Ctx<FF>::merkle_commit(const u64* leafs, size_t leaf_num, int ext, size_t lpn, size_t ic, u8* nodes_out, size_t cap, size_t* nn, u8* root); \
  template int Ctx<FF>::grind(const u8* seed, u32 bits, u64 start, u64 limit, u64* nonce);
MS_INSTANTIATE(GL)
MS_INSTANTIATE(BB)
#undef MS_INSTANTIATE

// the member templates other units call (trace / LDE commitments: EL = 1; FRI codewords: EL = the extension degree; ms_merkle_prove: both)
#define MS_INSTANTIATE_EL(FF, EL) \
  template int Ctx<FF>::tree_build<EL>(const Ctx<FF>::T*, size_t, size_t, size_t, u32, const Ctx<FF>::TreeShape&, DevBuf&, const msmerkle::LinColSpec*); \
  template int Ctx<FF>::tree_build_sharded<EL>(const Ctx<FF>::T*, size_t, size_t, size_t, u32, Ctx<FF>::TreeShape&, DevBuf&, const msmerkle::LinColSpec*);
MS_INSTANTIATE_EL(GL, 1)
MS_INSTANTIATE_EL(GL, 2)
MS_INSTANTIATE_EL(BB, 1)
MS_INSTANTIATE_EL(BB, 4)
#undef MS_INSTANTIATE_EL
template int Ctx<GL>::tree_build_sharded_contiguous<1>(const Ctx<GL>::T*, size_t, size_t, size_t, u32, Ctx<GL>::TreeShape&, DevBuf&);
template int Ctx<BB>::tree_build_sharded_contiguous<1>(const Ctx<BB>::T*, size_t, size_t, size_t, u32, Ctx<BB>::TreeShape&, DevBuf&);

}  // namespace msctx
