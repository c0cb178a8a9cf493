// mr_qentry.h — the entry of a pool kernel's ready queue (mr_pool.inc).
//
// A queue entry is one 32-bit LDS word:
//   lap << 16 | tcli << (SLOT_B + CLS_B + NODE_B) | node << (SLOT_B + CLS_B) | cls << SLOT_B | slot
// `slot` is the cluster's pool slot, `lap` the low 16 bits of the lap of the queue position the
// entry was written to (a claimer takes an entry only when its tag is the lap of the position it
// reserved), and (cls, node, tcli) the decision next_event made for the cluster's next event when
// the entry was published: the event's class, its node (a timer's or a delivery's destination;
// the service pool's clerk hosts included) and, for a tester-class event, whether a spawned thread
// runs. The claimer reads the decision from the entry it already waits for, so the event is
// decided once. Plain constexpr code without device types: a host program can walk every field
// (tests/test_pool_entry.py).
#pragma once
#include <stdint.h>

namespace mr {

struct QDec {  // next_event's decision
  uint32_t cls, node;
  bool tcli;
};
// FAM: the pool family, the unit's MR_POOL (1: the Raft pool, 512 slots, servers 0..6, no spawned
// threads; 2: the service pool, 256 slots, servers and clerk hosts 0..31, spawned threads)
template <uint32_t FAM>
struct QEntry {
  static_assert(FAM == 1u || FAM == 2u, "a pool family");
  static constexpr uint32_t SLOT_B = FAM == 2u ? 8u : 9u;  // log2 of the pool's slots
  static constexpr uint32_t CLS_B = 2u, NODE_B = FAM == 2u ? 5u : 3u, TCLI_B = FAM == 2u ? 1u : 0u;
  static constexpr uint32_t CLS_SH = SLOT_B, NODE_SH = CLS_SH + CLS_B, TCLI_SH = NODE_SH + NODE_B;
  static constexpr uint32_t LAP_SH = 16u;
  static_assert(TCLI_SH + TCLI_B <= LAP_SH, "slot and decision share the 16 bits below the lap tag");
  static constexpr uint32_t CLS_N = 1u << CLS_B, NODE_N = 1u << NODE_B, SLOT_N = 1u << SLOT_B;

  // the tag of queue position `pos`: what the entry written there carries above bit 16
  static constexpr uint32_t tag_of(uint32_t pos) { return (pos >> SLOT_B) << LAP_SH; }
  static constexpr uint32_t tag(uint32_t e) { return e & ~((1u << LAP_SH) - 1u); }
  static constexpr uint32_t pack(uint32_t pos, uint32_t slot, QDec d) {
    return tag_of(pos) | (TCLI_B && d.tcli ? 1u << TCLI_SH : 0u) | d.node << NODE_SH | d.cls << CLS_SH | slot;
  }
  static constexpr uint32_t slot(uint32_t e) { return e & (SLOT_N - 1u); }
  static constexpr QDec dec(uint32_t e) {
    return QDec{(e >> CLS_SH) & (CLS_N - 1u), (e >> NODE_SH) & (NODE_N - 1u),
                TCLI_B != 0u && ((e >> TCLI_SH) & 1u) != 0u};
  }
  // every value of one field, the others at both of their ends, comes back as it went in
  static constexpr bool round_trips() {
    const uint32_t pos_n = 1u << (32u - LAP_SH + SLOT_B);  // positions with distinct tags
    for (uint32_t lo = 0; lo < 2u; lo++) {
      const uint32_t c0 = lo ? CLS_N - 1u : 0u, n0 = lo ? NODE_N - 1u : 0u, s0 = lo ? SLOT_N - 1u : 0u;
      const uint32_t p0 = lo ? pos_n - 1u : 0u;
      const bool t0 = lo && TCLI_B;
      auto same = [](uint32_t pos, uint32_t s, QDec d) {
        const uint32_t e = pack(pos, s, d);
        const QDec r = dec(e);
        return tag(e) == tag_of(pos) && slot(e) == s && r.cls == d.cls && r.node == d.node && r.tcli == d.tcli;
      };
      for (uint32_t c = 0; c < CLS_N; c++)
        if (!same(p0, s0, QDec{c, n0, t0})) return false;
      for (uint32_t n = 0; n < NODE_N; n++)
        if (!same(p0, s0, QDec{c0, n, t0})) return false;
      for (uint32_t t = 0; t <= TCLI_B; t++)
        if (!same(p0, s0, QDec{c0, n0, t != 0u})) return false;
      for (uint32_t s = 0; s < SLOT_N; s++)
        if (!same(p0, s, QDec{c0, n0, t0})) return false;
      for (uint32_t l = 0; l < 16u; l++)  // each lap bit alone
        if (!same((1u << l) << SLOT_B | s0, s0, QDec{c0, n0, t0})) return false;
    }
    return true;
  }
};
static_assert(QEntry<1>::round_trips() && QEntry<2>::round_trips(), "a queue entry's fields do not overlap");

}  // namespace mr
