// mr_fork.inc — fork_kernel (mr_batch_fork, docs/SEMANTICS.md §12.5): positions of a destination
// batch become copies of positions of a source batch, row by row of MR_DEV_ARRAYS as the host's
// ForkPlan (mr_dev.h) lists them. Included by mr_kernel.hip's MR_COMMON unit; it reads no Dev.
//
// A bandwidth-bound broadcast: a few source clusters, many destinations. One launch covers every
// row; a block finds its row in the plan's block prefix (a scalar scan of at most FORK_ROWS
// entries) and then works by the row's kind:
//  * FK_MINOR, a cluster-minor matrix [fields][C]: a block takes 256 destination clusters and up
//    to FORK_FIELDS fields; thread t loads field[src_of[c]] (a gather over few distinct sources)
//    and stores field[c] (64 consecutive words per wave);
//  * FK_MAJOR, cluster-major records [owners][bytes]: whole slabs in 16-B quads, FORK_QUADS per
//    block: a slab of that many quads or more takes several blocks of one destination, smaller
//    slabs share a block. The source slab is read by every destination's block: it stays in L2.
//    A destination slab longer than the source's (a traced row of a larger trace_cap) is zero
//    above it, as a reset leaves it; a shorter one takes the source's head;
//  * FK_TAPE, the record tape [C][dcap]: as FK_MAJOR, but only the quads the source has drawn.
// A position whose src_of is FORK_SKIP is left alone. Every destination byte has one writer, and
// no source position is a destination (the host checked it), so there is nothing to order.
constexpr uint32_t FORK_U = FORK_QUADS / FORK_BLOCK;  // quads per thread: 16 KiB of a slab per block

template <class T>
DI void fork_minor(const ForkRow& R, const ForkPlan& P, uint32_t f0, uint32_t c, uint32_t s) {
  T* dst = reinterpret_cast<T*>(R.dst);
  const T* src = reinterpret_cast<const T*>(R.src);
  T v[FORK_FIELDS];
#pragma unroll
  for (uint32_t k = 0; k < FORK_FIELDS; k++)
    if (f0 + k < R.dper) v[k] = f0 + k == R.zfield ? T(0) : src[(size_t)(f0 + k) * P.Cs + s];
#pragma unroll
  for (uint32_t k = 0; k < FORK_FIELDS; k++)
    if (f0 + k < R.dper) dst[(size_t)(f0 + k) * P.Cd + c] = v[k];
}

// quads [q0, q0 + ..) of owner c's destination slab (Qd quads) from owner s's source slab, of
// which `have` quads count (the rest of the destination: zeros); thread-strided, loads first
DI void fork_quads(uint4* dst, const uint4* src, uint32_t Qd, uint32_t have, uint32_t q0, uint32_t end) {
  uint4 v[FORK_U];
#pragma unroll
  for (uint32_t u = 0; u < FORK_U; u++) {
    const uint32_t q = q0 + u * FORK_BLOCK + threadIdx.x;
    v[u] = q < end && q < have ? src[q] : make_uint4(0u, 0u, 0u, 0u);
  }
#pragma unroll
  for (uint32_t u = 0; u < FORK_U; u++) {
    const uint32_t q = q0 + u * FORK_BLOCK + threadIdx.x;
    if (q < end && q < Qd) dst[q] = v[u];
  }
}

__global__ void __launch_bounds__(FORK_BLOCK) fork_kernel(ForkPlan P) {
  uint32_t r = 0;
  while (r + 1 < P.n_rows && blockIdx.x >= P.row[r + 1].blk0) r++;  // (uniform: scalar loads)
  const ForkRow& R = P.row[r];
  const uint32_t b = blockIdx.x - R.blk0;
  if (R.kind == FK_MINOR) {
    const uint32_t nbc = (R.owners + FORK_BLOCK - 1) / FORK_BLOCK;
    const uint32_t f0 = b / nbc * FORK_FIELDS, c = b % nbc * FORK_BLOCK + threadIdx.x;
    if (c >= R.owners) return;
    const uint32_t s = P.src_of[c];
    if (s == FORK_SKIP) return;
    if (R.esz == 8) fork_minor<uint64_t>(R, P, f0, c, s);
    else fork_minor<uint32_t>(R, P, f0, c, s);
    return;
  }
  const uint32_t Qd = R.dper / 16u, Qs = R.sper / 16u;
  uint4* dst = reinterpret_cast<uint4*>(R.dst);
  const uint4* src = reinterpret_cast<const uint4*>(R.src);
  if (Qd >= FORK_QUADS || R.kind == FK_TAPE) {  // blocks per owner: a slab chunk each
    const uint32_t bpo = (Qd + FORK_QUADS - 1) / FORK_QUADS;
    const uint32_t c = b / bpo, q0 = b % bpo * FORK_QUADS;
    if (c >= R.owners) return;
    const uint32_t s = P.src_of[c];
    if (s == FORK_SKIP) return;
    uint32_t have = Qs, end = Qd;
    if (R.kind == FK_TAPE) {  // the records the source keeps; the destination's rest stays unread
      const uint32_t used = P.tape_used[s];
      have = used < Qs ? used : Qs;
      end = have < Qd ? have : Qd;
      if (q0 >= end) return;
    }
    fork_quads(dst + (size_t)c * Qd, src + (size_t)s * Qs, Qd, have, q0, end);
  } else {  // owners per block: whole small slabs
    const uint32_t opb = FORK_QUADS / Qd;
    uint4 v[FORK_U];
    uint32_t at[FORK_U];  // the destination quad within the row's owner c, ~0u: none
    size_t co[FORK_U];
#pragma unroll
    for (uint32_t u = 0; u < FORK_U; u++) {
      const uint32_t i = u * FORK_BLOCK + threadIdx.x, o = i / Qd, q = i - o * Qd;
      const uint32_t c = b * opb + o;
      at[u] = ~0u;
      co[u] = c;
      if (o >= opb || c >= R.owners) continue;
      const uint32_t s = P.src_of[c];
      if (s == FORK_SKIP) continue;
      at[u] = q;
      v[u] = q < Qs ? src[(size_t)s * Qs + q] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (uint32_t u = 0; u < FORK_U; u++)
      if (at[u] != ~0u) dst[co[u] * Qd + at[u]] = v[u];
  }
}

// the launch's blocks: the plan's total (the host laid the rows' prefixes out with fork_blocks)
hipError_t launch_fork(const ForkPlan& P, hipStream_t s) {
  if (!P.blocks) return hipSuccess;
  hipLaunchKernelGGL(fork_kernel, dim3(P.blocks), dim3(FORK_BLOCK), 0, s, P);
  return hipGetLastError();
}
