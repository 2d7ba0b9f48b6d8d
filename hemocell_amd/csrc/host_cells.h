// The host's view of the cells of one type (hc_cells::host[t]).  Standard library only: the CPU test builds it alone.
//
// Invariants:
//  - ids is always current, in slot order: the device's books change it without touching the rest (the id-only edits below).
//  - The payload -- every other array -- is held only from sync_to_host until sync_to_device (hc_cells::host_dirty covers the
//    second half of that span); outside it the payload arrays keep stale sizes and contents and nobody reads them.
//  - Whenever the payload is held, every payload array is sized to ids.size(): pos, vel, frc 3 * nv per cell ([cell][vertex][xyz]);
//    tag 1 per cell (0 complete, 2 incomplete; a gone cell, 1, lives only until compact drops it); dead nv per cell (1 = this
//    particle was removed, reference deletion mode); sflag nv per cell (1 = the particle carries the solidify flag);
//    rep (force_repulsion) 3 * nv per cell if and only if has_rep, else empty.
//  - No code outside this struct infers anything from a vector's size: has_rep says whether rep is there, cells() how many.
// cells() and hc_cells::ncells[t] are two numbers on purpose: ncells is what the device regions hold, and the two differ while
// host_dirty is set (cells appended or compacted on the host and not yet uploaded).
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

struct HostCells {
  int nv = 0;   // vertices per cell (set once, when the type joins the container)
  std::vector<long> ids;
  std::vector<double> pos, vel, frc, rep;
  std::vector<int> tag;
  std::vector<unsigned char> dead, sflag;
  bool has_rep = false;

  size_t cells() const { return ids.size(); }

  // ---- id-only edits: the payload is NOT held here (the device has the cells; only the books change)
  void ids_push(long id) { ids.push_back(id); }
  void ids_move(size_t dst, size_t src) { ids[dst] = ids[src]; }   // fill the hole at dst with the cell at src
  void ids_truncate(size_t n) { ids.resize(n); }

  // ---- payload held from here on.  fit: every payload array to the size the ids ask for, what is new is zero
  void fit() {
    const size_t n = cells() * (size_t)nv;
    pos.resize(3 * n, 0.0); vel.resize(3 * n, 0.0); frc.resize(3 * n, 0.0); rep.resize(has_rep ? 3 * n : 0, 0.0);
    tag.resize(cells(), 0); dead.resize(n, 0); sflag.resize(n, 0);
  }
  // for a download of cells() cells: tag, dead, sflag and rep zeroed (all complete, all live, none flagged), pos / vel / frc to be overwritten
  void size_payload(bool with_rep) { has_rep = with_rep; rep.clear(); tag.clear(); dead.clear(); sflag.clear(); fit(); }
  // one more cell, zero in every array; returns its positions [nv][3] for the caller to write.  A repulsion enabled since
  // the payload was taken (with_rep and not yet has_rep) gives the cells already here a zero force_repulsion.
  double *append(long id, bool with_rep) {
    if (with_rep != has_rep) { has_rep = with_rep; rep.clear(); fit(); }
    ids.push_back(id); fit();
    return pos.data() + 3 * (cells() - 1) * (size_t)nv;
  }
  // stable compaction: keep(slot) is asked once per slot, in ascending order; the kept cells close up in every array and
  // keep their order.  Returns the new count.
  template <class Keep>
  size_t compact(Keep keep) {
    const size_t nc = cells(), k = (size_t)nv;
    size_t w = 0, c = 0;
    auto move = [&](std::vector<double> &v) { std::copy(v.begin() + 3 * c * k, v.begin() + 3 * (c + 1) * k, v.begin() + 3 * w * k); };
    for (; c < nc; c++) {
      if (!keep(c)) continue;
      if (w != c) {
        move(pos); move(vel); move(frc); if (has_rep) move(rep);
        std::copy(dead.begin() + c * k, dead.begin() + (c + 1) * k, dead.begin() + w * k);
        std::copy(sflag.begin() + c * k, sflag.begin() + (c + 1) * k, sflag.begin() + w * k);
        tag[w] = tag[c]; ids[w] = ids[c];
      }
      w++;
    }
    ids.resize(w); fit();
    return w;
  }
};
