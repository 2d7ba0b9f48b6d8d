"""numpy restatement of the pre-inlet's cell injection and outflow sink (csrc/preinlet.hip, hcp_preinlet_apply) on the public
record API: Cells.records() / set_records() (the reference's 120-byte particle record) and nothing else.

A cell of the periodic pre-inlet keeps unwrapped positions: after `lap` turns round the Lp nodes of the inlet axis it sits at
lap * Lp + (its place in the box).  Per complete cell, with cmin / cmax the extent of its vertices on the axis:

    lap  = floor(cmin / Lp)
    in   = cmin - lap * Lp >= window_lo  and  cmax - lap * Lp <= window_hi
    id'  = id + (lap - orientation) * id_stride          (orientation -1: *neg, +1: *pos)
    p'   = p + shift, on the axis p + (shift[axis] - lap * Lp)

in the operand order of the kernels (doubles throughout, lap converted to double before it is multiplied).  Candidates are
taken in ascending (type, slot) order -- the order of records() -- and one is skipped when id' was offered before, counted
rejected when its shifted extents leave [0, n - 1] of the domain on any axis, and skipped when the domain holds id'; the rest
are appended to the domain's records.  The sink drops the domain's cells with cmax > plane (*neg) or cmin < plane (*pos).
Partly arrived cells are never added (the recorded deviation from helper/preInlet.cpp:254-351)."""
import numpy as np


def cells_of(rec):
    """[(type, id, indices of the cell's records in vertexId order)] in ascending (type, slot) order: types ascending, cells of
    a type in the order of their first record"""
    out, seen = [], {}
    for k in range(len(rec)):
        key = (int(rec["celltype"][k]), int(rec["cellId"][k]))
        if key not in seen:
            seen[key] = len(out)
            out.append([key[0], key[1], []])
        out[seen[key]][2].append(k)
    out.sort(key=lambda c: c[0])   # stable: slot order within a type stays
    return [(t, i, np.array(sorted(idx, key=lambda k: int(rec["vertexId"][k])), dtype=np.int64)) for t, i, idx in out]


def canonical(rec):
    """the records in the order records() lists them: types ascending, cells in slot order, vertices ascending"""
    cells = cells_of(rec)
    return np.concatenate([rec[idx] for _, _, idx in cells]) if cells else rec[:0].copy()


def by_id(rec):
    """{(type, id): the cell's records in vertex order}"""
    return {(t, i): rec[idx] for t, i, idx in cells_of(rec)}


def lap_and_window(cmin, cmax, Lp, window):
    """(lap, inside) of one cell from its extent on the axis"""
    Lp = np.float64(Lp)
    cmin, cmax = np.float64(cmin), np.float64(cmax)
    lap = int(np.floor(cmin / Lp))
    inside = bool(cmin - np.float64(lap) * Lp >= np.float64(window[0]) and cmax - np.float64(lap) * Lp <= np.float64(window[1]))
    return lap, inside


def new_id(cell_id, lap, orientation, id_stride):
    return int(cell_id) + (int(lap) - int(orientation)) * int(id_stride)


def translation(lap, axis, Lp, shift):
    """the three addends of a cell's positions"""
    t = [np.float64(shift[0]), np.float64(shift[1]), np.float64(shift[2])]
    t[axis] = np.float64(shift[axis]) - np.float64(lap) * np.float64(Lp)
    return t


def select(rec, nv, axis, Lp, window):
    """the candidates of a container's records: [(type, id, indices, lap)] of its complete cells that lie wholly in the window;
    nv: vertices per cell of each type"""
    out = []
    for t, cid, idx in cells_of(rec):
        if len(idx) != nv[t]:
            continue   # incomplete: never a candidate
        x = rec["position"][idx, axis]
        lap, inside = lap_and_window(x.min(), x.max(), Lp, window)
        if inside:
            out.append((t, cid, idx, lap))
    return out


def shifted(rec, idx, lap, axis, Lp, shift, cell_id):
    """the records of one cell as they arrive in the domain"""
    new = rec[idx].copy()
    t = translation(lap, axis, Lp, shift)
    for d in range(3):
        new["position"][:, d] = rec["position"][idx, d] + t[d]
    new["cellId"] = cell_id
    new["restime"] = 0
    return new


def inject(pre_rec, dom_rec, nv, axis, orientation, Lp, window, shift, id_stride, dom_dims, offered):
    """one injection: returns (the domain's records with the arrivals appended, ids injected, number rejected).  offered: the
    set of (type, id') offered so far; updated in place"""
    held = set((int(t), int(i)) for t, i in zip(dom_rec["celltype"], dom_rec["cellId"]))
    arrivals, ids, rejected = [], [], 0
    for t, cid, idx, lap in select(pre_rec, nv, axis, Lp, window):
        nid = new_id(cid, lap, orientation, id_stride)
        if (t, nid) in offered:
            continue
        offered.add((t, nid))
        tr = translation(lap, axis, Lp, shift)
        p = pre_rec["position"][idx]
        inside = all(p[:, d].min() + tr[d] >= 0.0 and p[:, d].max() + tr[d] <= np.float64(dom_dims[d] - 1) for d in range(3))
        if not inside:
            rejected += 1
            continue
        if (t, nid) in held:
            continue
        held.add((t, nid))
        arrivals.append(shifted(pre_rec, idx, lap, axis, Lp, shift, nid))
        ids.append((t, nid))
    if not arrivals:
        return dom_rec, ids, rejected
    # a type's arrivals follow the cells that type already holds; set_records keeps the order of first records within a type
    return np.concatenate([dom_rec] + arrivals), ids, rejected


def sink(dom_rec, axis, orientation, plane):
    """the domain's records without the cells that reach past the plane downstream; returns (records, ids removed)"""
    keep = np.ones(len(dom_rec), bool)
    gone = []
    for t, cid, idx in cells_of(dom_rec):
        x = dom_rec["position"][idx, axis]
        if (x.max() > plane) if orientation < 0 else (x.min() < plane):
            keep[idx] = False
            gone.append((t, cid))
    return dom_rec[keep], gone
