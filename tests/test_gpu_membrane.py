"""mechanics_kernel<MODEL, SEPARATE, MD> in the states of tests/membrane_states.py: large strain, both sides of every pole,
the viscosity cap, the folded platelet, the WBC thresholds, an incomplete cell.  All four models, both instantiations:

  RBC_HO       the product mesh, 642 vertices, MD 8; eta_m 0 and 5e-10
  PLT_SIMPLE   its mesh, 66 vertices, the 128-thread launch, MD 8; eta_m 5e-10
  WBC_HO       wbc_sphere, 642 vertices, MD 8; eta_m 5e-10 and 0
  RBC_MALARIA  the gametocyte STL, 1507 vertices, the wide tables (MD 16); eta_m 5e-10 and 0; kInnerLink 7 (the fixture has
               kInnerLink = kLink, which would hide the one modulus taken for the other)

Two cells per type on a 64 x 48 x 48 periodic lattice; one mechanics launch and one component launch per state.

Against the oracle: bit for bit in every state (RBC: components 0-4 and the unified force, WBC and malaria: components 0-4;
PLT within 1e-12 of the largest force, its atan2 not being glibc's).  Against the restatement (tests/membrane_ref.py): every
component and the unified force within K 2^-53 abs, K as fixed in tests/test_membrane_cpu.py; WBC and malaria take RBC's K
for components 0-4.  K of their inner links is measured in the same way, from the double-precision loops of
tests/test_gpu_wbc.py / test_gpu_malaria.py against the restatement over all states (largest ratio 3.30e4 for WBC, in
wbc_radius where 1 - l / d cancels to 1e-5, and 2.91e4 for malaria; times four, rounded up: 262144 and 131072); their unified
force takes the larger of RBC's unified K and that.

The state checkers (S.check) run before any force is compared.  The mutation controls of the CPU test fail by the same
factor against the GPU's values.  '<=' for '<' at a WBC threshold is the one slip no force can show: at l == d the term is
(1 - l / d) k == 0 exactly, so the wrong restatement is the same function; the test asserts that identity, that the edge
with l == d exactly contributes exact zeros on the GPU, and that the edges 1e-5 below and above fire and do not.
"""
import numpy as np
import pytest

from oracle import oracle as O
from tests import membrane_ref as M
from tests import membrane_states as S
from tests.test_membrane_cpu import K as K_CPU, MUTANTS as MUTANTS_CPU, STATES as STATES_CPU
from tests.test_gpu_malaria import STLS, _OracleType, _inner_links as _malaria_links
from tests.test_gpu_wbc import WBC_XML, _inner_links as _wbc_links

pytestmark = pytest.mark.gpu

K_INNER = {"wbc": 262144.0, "malaria": 131072.0}
K = dict(K_CPU)
for _m in K_INNER:
    K[_m] = K_CPU["rbc"][:5] + (K_INNER[_m], max(K_CPU["rbc"][6], K_INNER[_m]))

HO = STATES_CPU["rbc_visc"]
STATES = dict(STATES_CPU, wbc=HO + ["wbc_radius", "wbc_core"], wbc_eta0=["moderate"], malaria=HO, malaria_eta0=["moderate"])
CASES = [(case, st) for case in STATES for st in STATES[case]]
_HO_MUTANTS = (("no_fabs_volume", "volume_plus", 0), ("no_fabs_volume", "volume_minus", 0), ("no_fabs_area", "area_plus", 1),
               ("no_fabs_area", "area_minus", 1), ("no_fabs_bending", "bending_plus", 2), ("no_fabs_bending", "bending_minus", 2),
               ("no_fabs_link", "link_plus", 3), ("no_visc_cap", "visc_cap", 4), ("cap_per_component", "visc_cap", 4),
               ("ring_share_over_6", "moderate", 2))
MUTANTS = {w: list(v) for w, v in MUTANTS_CPU.items()}
for _case in ("wbc", "malaria"):
    for _w, _s, _j in _HO_MUTANTS:
        MUTANTS[_w].append((_case, _s, _j))
MUTANTS["malaria_inner_k_link"] = [("malaria", "moderate", 5)]


def _make_type(gpu, P, case):
    model = case.split("_")[0]
    eta = 0.0 if case in ("rbc", "wbc_eta0", "malaria_eta0") else 5e-10
    if model == "rbc":
        return gpu.CellType.rbc(P, eta_m=eta)
    if model == "plt":
        return gpu.CellType.plt(P, eta_m=eta)
    if model == "wbc":
        return gpu.CellType.wbc(P, xml=WBC_XML, eta_m=eta)
    return gpu.CellType.malaria(P, stl=STLS["stretch"], eta_m=eta, kInnerLink=7.0)


class _Case:
    def __init__(self, orc, gpu, case):
        self.orc, self.case, self.model = orc, case, case.split("_")[0]
        P = gpu.base_parameters()
        self.T = _make_type(gpu, P, case)
        self.nv = self.T.nv
        self.ot = _OracleType(self.T)                  # the product's tables as an orc_celltype, RBC_HO law, no inner links
        self.tab = dict(self.ot.keep, inner_edges=self.ot.inner, inner_edge_length_eq=self.ot.inner_len_eq)
        self.tab.update({k: self.ot.tables[k] for k in ("volume_eq", "area_mean_eq", "edge_mean_eq", "k_volume", "k_area", "k_link", "k_bend", "eta_m")})
        self.tab.update(self.T.wbc_constants() if self.model == "wbc" else self.T.malaria_constants() if self.model == "malaria" else {})
        if self.model in ("rbc", "plt"):               # the oracle's own type: its tables are the product's (test_parameters_and_tables_match_oracle)
            Po = O.make_params(orc)
            self.To = (O.make_rbc if self.model == "rbc" else O.make_plt)(orc, Po, eta_m=0.0 if case == "rbc" else 5e-10)
            assert self.To.contents.eta_m == self.tab["eta_m"]
            self.flags = 0x1f
        else:
            self.To, self.flags = self.ot.ptr, 0x0f
        self.L = gpu.Lattice(64, 48, 48, (1, 1, 1), 1.0)
        self.cells = gpu.Cells(self.L, P)
        self.t = self.cells.addCellType(self.T, 1)
        for c, a in ((S.CENTRES[0], (0, 0, 0)), (S.CENTRES[1], (35.0, 10.0, -70.0))):
            assert self.cells.addCell(self.t, c, a)
        self.states = S.build(self.tab, self.model, self.cells.positions.reshape(2, self.nv, 3))
        if case.endswith("eta0"):
            self.states = {"moderate": self.states["moderate"]}
        assert sorted(self.states) == sorted(STATES[case]), sorted(self.states)
        self._ref, self._gpu, self._orc = {}, {}, {}

    def ref(self, name):
        if name not in self._ref:
            self._ref[name] = S.check(self.tab, self.model, self.states[name])
        return self._ref[name]

    def device(self, name):
        """-> (unified force [2][nv][3] of the unified kernel, components [6][2][nv][3] of the SEPARATE kernel)"""
        if name not in self._gpu:
            st = self.states[name]
            self.cells.positions = st.pos.reshape(-1, 3); self.cells.velocities = st.vel.reshape(-1, 3)
            self.cells.applyConstitutiveModel(0, True)
            self._gpu[name] = (self.cells.forces.reshape(2, self.nv, 3), self.cells.force_components(self.t).reshape(6, 2, self.nv, 3))
        return self._gpu[name]

    def oracle(self, name):
        if name not in self._orc:
            st, out = self.states[name], []
            for c in range(2):
                co, fo = np.zeros((6, self.nv, 3)), np.zeros((self.nv, 3))
                self.orc.orc_cell_forces(self.To, O.dptr(st.pos[c]), O.dptr(st.vel[c]), O.dptr(np.zeros((self.nv, 3))), O.dptr(co), self.flags)
                self.orc.orc_cell_forces(self.To, O.dptr(st.pos[c]), O.dptr(st.vel[c]), O.dptr(fo), None, self.flags)
                out.append((co, fo))
            self._orc[name] = out
        return self._orc[name]

    def loops(self, name, c):
        """the inner links of WBC / malaria from the double-precision loops of their own test files"""
        p = self.states[name].pos[c]
        if self.model == "wbc":
            return _wbc_links(self.ot.inner, p, self.tab)[0]
        return _malaria_links(self.ot.inner, self.ot.inner_len_eq, p, self.tab["k_inner_link"])

    def destroy(self):
        self.cells.destroy(); self.L.destroy(); self.T.destroy()


@pytest.fixture(scope="module")
def cases(orc, gpu):
    made = {}

    def get(case):
        if case not in made:
            made[case] = _Case(orc, gpu, case)
        return made[case]
    yield get
    for cs in made.values():
        cs.destroy()


@pytest.mark.parametrize("case,state", CASES)
def test_forces_against_oracle_and_restatement(cases, case, state):
    cs = cases(case)
    ref = cs.ref(state)                                # the state's checker, before any force is compared
    fg, comp = cs.device(state)
    orc = cs.oracle(state)
    r = np.zeros(7)
    for c in range(2):
        co, fo = orc[c]
        if cs.model == "plt":
            scale = np.abs(fo).max()
            assert np.abs(fg[c] - fo).max() <= 1e-12 * scale and np.abs(comp[:, c] - co).max() <= 1e-12 * scale
        else:
            for j in range(5):
                assert np.array_equal(comp[j, c], co[j]), (j, np.abs(comp[j, c] - co[j]).max())
            if cs.model == "rbc":
                assert np.array_equal(fg[c], fo), np.abs(fg[c] - fo).max()
                assert not comp[5, c].any()
            else:
                assert np.array_equal(comp[5, c], cs.loops(state, c))
        for j in range(6):
            r[j] = max(r[j], M.ratio(comp[j, c], ref[c]["comp"][j], ref[c]["comp_abs"][j]))
        r[6] = max(r[6], M.ratio(fg[c], ref[c]["force"], ref[c]["force_abs"]))
        if cs.tab["eta_m"] == 0.0:
            assert not comp[4, c].any() and not ref[c]["comp_abs"][4].any()      # exact zeros, whatever the velocities
    print("%s/%s ratios %s" % (case, state, " ".join("%.3g" % v for v in r)))
    assert (r <= np.array(K[cs.model])).all(), r


@pytest.mark.parametrize("state", ["wbc_radius", "wbc_core"])
def test_wbc_edge_at_the_threshold_adds_nothing(cases, state):
    cs = cases("wbc")
    st, ref = cs.states[state], cs.ref(state)
    _, comp = cs.device(state)
    a, b = cs.ot.inner[st.claim["exact_edge"]]
    assert ((cs.ot.inner == a) | (cs.ot.inner == b)).sum() == 2          # no other inner edge at these two vertices
    k, d = cs.tab, st.claim["threshold"]
    if state == "wbc_radius":                                            # neither term: l == 2 radius > 2 core_radius
        assert not comp[5, 0, a].any() and not comp[5, 0, b].any()
    else:                                                                # the cytoskeleton term alone, along x
        ux = np.sign(st.pos[0][b, 0] - st.pos[0][a, 0])
        f = (ux * (1.0 - (d / (2 * k["radius"])))) * k["k_cytoskeleton"]
        assert np.array_equal(comp[5, 0, a], [-f, 0.0, 0.0]) and np.array_equal(comp[5, 0, b], [f, 0.0, 0.0])
    # '<=' for '<' is the same function: (1 - l / d) k == 0 at l == d
    for c in range(2):
        bad = M.forces(cs.tab, st.pos[c], st.vel[c], "wbc", wrong="wbc_le_" + st.claim["which"])
        assert bad["info"]["fired_" + st.claim["which"]].sum() == ref[c]["info"]["fired_" + st.claim["which"]].sum() + (c == 0)
        assert np.array_equal(bad["comp"], ref[c]["comp"]) and np.array_equal(bad["comp_abs"], ref[c]["comp_abs"])


@pytest.mark.parametrize("model", ["wbc", "malaria"])
def test_inner_link_k_of_the_loops(cases, model):
    """K_INNER: the double-precision loops against the restatement, over all states, with the room K was fixed with"""
    cs = cases(model)
    worst = max(M.ratio(cs.loops(s, c), cs.ref(s)[c]["comp"][5], cs.ref(s)[c]["comp_abs"][5]) for s in STATES[model] for c in range(2))
    print("%s inner links: loops against restatement %.4g, K %g" % (model, worst, K_INNER[model]))
    assert 2 * worst <= K_INNER[model]


@pytest.mark.parametrize("wrong", list(MUTANTS))
def test_mutant_restatement_is_far_outside_the_bound(cases, wrong):
    for case, state, j in MUTANTS[wrong]:
        cs = cases(case)
        ref, st = cs.ref(state), cs.states[state]
        _, comp = cs.device(state)
        far = 0.0
        for c in range(2):
            bad = M.forces(cs.tab, st.pos[c], st.vel[c], cs.model, wrong=wrong)
            far = max(far, M.ratio(comp[j, c], bad["comp"][j], ref[c]["comp_abs"][j]) / K[cs.model][j])
        print("%s in %s/%s: %.3g bounds away" % (wrong, case, state, far))
        assert far >= 1000.0, (wrong, case, state, far)


def test_incomplete_cell_gets_exact_zeros_in_both_modes(orc, gpu):
    """a cell that lost particles at a wall (tag 2): its unified force and all six components are exact zeros, and the
    complete cell beside it carries the bits it carries alone"""
    from tests.test_gpu_observables import _incomplete_pair
    Lo, Lg, hg, cf, nv = _incomplete_pair(orc, gpu)
    try:
        alive = cf.alive()
        assert alive[:nv].all() and not alive[nv:].all()
        pos, vel = cf.positions, cf.velocities
        cf.forces = np.full((2 * nv, 3), 7.0)            # whatever was there has to go
        cf.applyConstitutiveModel(0, True)
        f, comp = cf.forces, cf.force_components(0)
        assert not f[nv:].any() and not comp[:, nv:].any()
        assert f[:nv].any() and comp[:4, :nv].any(axis=(1, 2)).all()
    finally:
        Lo.destroy(); Lg.destroy()
    P = gpu.base_parameters()
    T = gpu.CellType.rbc(P)
    L = gpu.Lattice(40, 34, 34, (1, 0, 0), 1.0)
    alone = gpu.Cells(L, P)
    t = alone.addCellType(T, 1)
    assert alone.addCell(t, (12.0, 16.5, 16.5), (90, 0, 0))
    alone.positions = pos[:nv]; alone.velocities = vel[:nv]
    alone.applyConstitutiveModel(0, True)
    assert np.array_equal(alone.forces, f[:nv]) and np.array_equal(alone.force_components(t), comp[:, :nv])
    alone.destroy(); L.destroy(); T.destroy()
