"""The element building blocks of csrc/element.hpp that more than one kernel now runs through, at the block edges where
a shared shell can go wrong: the c3d4 record -> tangent shell (tet4_tangent_index / tet4_tangent_store /
tet4_force_store) under fem_tet4_nl and fem_tet4_j2, and point_stress / the merged stress kernels under the plain and
the thermal stress entry points. Behaviour only, every comparison bitwise; nothing here depends on how the code is laid
out.

Tangent kernels (64 elements per workgroup), M in {1, 63, 64, 65, 129} elements of mesh.kuhn_cube(3, jitter=0.15)
(162 tets), both hyperelastic materials on the seeded random field of the nonlinear tests and J2 on the `graded` field
of the plasticity tests with the element list reversed (every element of the first 66 yields; of the first 129, 108
yield and 21 stay elastic -- counted on the CPU restatement):
  * the full tangent is the packed one with its blocks mirrored, and equals its own transpose;
  * the Kt == NULL launch gives the forces, energies, stresses (and state) of the tangent launch;
  * prefix: the first M elements of an (M + 1)-element launch equal the M-element launch;
  * no overrun: every output buffer carries one more element's worth of a sentinel, which stays untouched.

Stress kernels (256 elements per workgroup / tile), c3d4 with M in {255, 256, 257} of kuhn_cube(4) (384 tets), c3d6 and
c3d8 with M = 257 of wedge_box(6) (432) / hex_box(7) (343), single and per-point layout, T == T_ref given as a float,
per node and per element: the prefix and sentinel properties for the plain and the thermal entry point, the public
functions against the raw launches, and on c3d4 the thermal entry point returns the plain one's tensors and von Mises
under torch.equal (which takes -0.0 for 0.0, the only thing the subtraction of a zero thermal strain can change).
c3d6 / c3d8 are left out of that last comparison: there the two entry points have differed in the last bits since the
thermal one was added (measured on these cases: 25-30 % of the tensor entries differ, by at most half an ulp of the
largest entry) -- the compiler contracts point_stress's sums of two products (g_y u_x + g_x u_y) into a multiply and a
fused multiply-add in the other order in the thermal kernel, whose node gather is its own loop."""
import functools

import pytest
import torch

import hyperelastic_ref as HR
import plasticity_ref as PR

pytestmark = pytest.mark.gpu

F64 = torch.float64
SENT = -1.2345678901234567e300   # no output of these kernels on these inputs
BLOCK_MS = (1, 63, 64, 65, 129)
KERNELS = ("svk", "neo_hookean", "j2")
E_, NU_, ALPHA, T_REF = 1.0, 0.3, 1.2e-5, 20.0


def sentinel(dev, *shape, dtype=F64):
    return torch.full(shape, 255 if dtype == torch.uint8 else SENT, dtype=dtype, device=dev)


def split_tail(out, rows):
    """{name: first `rows[name]` rows on the host}; asserts that everything past them is still the sentinel."""
    res = {}
    for k, v in out.items():
        v = v.cpu()
        n = rows[k] if isinstance(rows, dict) else rows
        assert v.shape[0] > n
        assert torch.equal(v[n:], sentinel("cpu", *v[n:].shape, dtype=v.dtype)), f"{k}: written past element {n}"
        res[k] = v[:n]
    return res


# ---------------------------------------------------------------- c3d4 tangent shell
@functools.lru_cache(maxsize=None)
def tet_case(kernel):
    """(coords, tets, u) on the host, formed once and never modified."""
    from fem355 import mesh
    c, t = mesh.kuhn_cube(3, jitter=0.15)
    c = c.to(F64)
    if kernel == "j2":
        E, nu, sy, _ = PR.material("unit")
        return c, t.flip(0).contiguous(), PR.field("graded", c, 3, PR.yield_strain(E, nu, sy))
    return c, t, HR.field("random", c, 3)


def tangent_launch(dev, kernel, M, packed, tangent=True):
    """One raw launch on the first M elements, every output one element longer than M and filled with the sentinel."""
    from fem355 import _capi as C
    lib = C.lib()
    c, t, u = tet_case(kernel)
    cd, td, ud = c.to(dev), t[:M].contiguous().to(dev), u.to(dev)
    S = int(lib.fem_ke_sym_stride(4))
    out = dict(Kt=sentinel(dev, M + 1, S) if packed else sentinel(dev, M + 1, 12, 12), fe=sentinel(dev, M + 1, 4, 3),
               we=sentinel(dev, M + 1), sigma=sentinel(dev, M + 1, 6))
    kt = C.ptr(out["Kt"]) if tangent else None
    st = C.stream(torch.device(dev))
    if kernel == "j2":
        E, nu, sy, H = PR.material("unit")
        out.update(ep=sentinel(dev, M + 1, 6), alpha=sentinel(dev, M + 1),
                   plastic=sentinel(dev, M + 1, dtype=torch.uint8))
        bad = torch.full((1,), M, dtype=torch.int64, device=dev)
        C.check(lib.fem_tet4_j2(C.ptr(cd), C.ptr(td), M, C.ptr(ud), E, nu, sy, H, None, None, 1 if packed else 0, kt,
                                C.ptr(out["fe"]), C.ptr(out["we"]), C.ptr(out["sigma"]), C.ptr(out["ep"]),
                                C.ptr(out["alpha"]), C.ptr(out["plastic"]), C.ptr(bad), st), "fem_tet4_j2")
    else:
        out.update(detF=sentinel(dev, M + 1))
        bad = torch.full((2,), M, dtype=torch.int64, device=dev)
        C.check(lib.fem_tet4_nl(C.ptr(cd), C.ptr(td), M, C.ptr(ud), E_, NU_, C.MATERIALS[kernel], 1 if packed else 0,
                                kt, C.ptr(out["fe"]), C.ptr(out["we"]), C.ptr(out["sigma"]), C.ptr(out["detF"]),
                                C.ptr(bad[0:1]), C.ptr(bad[1:2]), st), "fem_tet4_nl")
    torch.cuda.synchronize()
    assert bool((bad.cpu() == M).all()), "a degenerate or inverted element in the test mesh"
    rows = {k: (0 if k == "Kt" and not tangent else M) for k in out}
    return split_tail(out, rows)


@pytest.mark.parametrize("M", BLOCK_MS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_tangent_shell(gpu, kernel, M):
    full = tangent_launch(gpu, kernel, M, packed=False)
    pk = tangent_launch(gpu, kernel, M, packed=True)
    nt = tangent_launch(gpu, kernel, M, packed=False, tangent=False)
    rest = [k for k in full if k != "Kt"]
    if kernel == "j2":
        assert bool(full["plastic"].any()), "no element yields"
        if M == 129:
            assert not bool(full["plastic"].all()), "no element stays elastic"
    else:
        assert float(full["fe"].abs().max()) > 0.0
    # full == packed mirrored == its own transpose
    blk = 0
    for a in range(4):
        for b in range(a, 4):
            p = pk["Kt"][:, 9 * blk: 9 * blk + 9].reshape(M, 3, 3)
            assert torch.equal(full["Kt"][:, 3 * a: 3 * a + 3, 3 * b: 3 * b + 3], p), (a, b)
            assert torch.equal(full["Kt"][:, 3 * b: 3 * b + 3, 3 * a: 3 * a + 3], p.transpose(1, 2)), (b, a)
            blk += 1
    assert torch.equal(full["Kt"], full["Kt"].transpose(1, 2))
    for k in rest:
        assert torch.equal(nt[k], full[k]) and torch.equal(pk[k], full[k]), k
    # prefix: element M of a longer launch changes nothing before it
    for packed, tangent, ref in ((False, True, full), (True, True, pk), (False, False, nt)):
        more = tangent_launch(gpu, kernel, M + 1, packed=packed, tangent=tangent)
        for k in ref:
            assert torch.equal(more[k][:ref[k].shape[0]], ref[k]), (k, packed, tangent)


# ---------------------------------------------------------------- stress kernels, thermal option
STRESS_CASES = (("c3d4", 255), ("c3d4", 256), ("c3d4", 257), ("c3d6", 257), ("c3d8", 257))
NPE = {"c3d4": 4, "c3d6": 6, "c3d8": 8}


@functools.lru_cache(maxsize=None)
def stress_case(et):
    from fem355 import mesh
    c, el = {"c3d4": lambda: mesh.kuhn_cube(4, jitter=0.15), "c3d6": lambda: mesh.wedge_box(6, jitter=0.1),
             "c3d8": lambda: mesh.hex_box(7, jitter=0.1)}[et]()
    c = c.to(F64)
    u = 1e-3 * (2.0 * torch.rand(c.shape, dtype=F64, generator=torch.Generator().manual_seed(11)) - 1.0)
    return c, el, u


def temperature(mode, N, M, dev):
    """T == T_ref in the three forms the entry points read -> (array, FEM_LOAD_* mode)."""
    from fem355 import _capi as C
    n = {"uniform": 1, "nodal": N, "element": M}[mode]
    return torch.full((n,), T_REF, dtype=F64, device=dev), {"uniform": C.LOAD_UNIFORM, "nodal": C.LOAD_NODAL,
                                                             "element": C.LOAD_ELEMENT}[mode]


def stress_launch(dev, et, M, single, tmode=None):
    """One raw launch of the plain (tmode None) or the thermal entry point on the first M elements; the outputs are one
    element's slots longer than the launch's and filled with the sentinel."""
    from fem355 import _capi as C, element as EL, loads as LD
    lib = C.lib()
    c, el, u = stress_case(et)
    cd, ed, ud = c.to(dev), el[:M].contiguous().to(dev), u.to(dev)
    st = C.stream(torch.device(dev))
    if tmode is not None:
        Td, tm = temperature(tmode, c.shape[0], M, dev)
    if et == "c3d4":
        per = 1
        out = dict(sig=sentinel(dev, M + 1, 3, 3), vm=sentinel(dev, M + 1))
        bad = torch.full((1,), M, dtype=torch.int64, device=dev)
        if tmode is None:
            C.check(lib.fem_tet4_stress(C.ptr(cd), C.ptr(ed), M, C.ptr(ud), E_, NU_, C.ptr(out["sig"]),
                                        C.ptr(out["vm"]), C.ptr(bad), st), "fem_tet4_stress")
        else:
            C.check(lib.fem_tet4_stress_thermal(C.ptr(cd), C.ptr(ed), M, C.ptr(ud), E_, NU_, ALPHA, C.ptr(Td), tm,
                                                T_REF, C.ptr(out["sig"]), C.ptr(out["vm"]), C.ptr(bad), st),
                    "fem_tet4_stress_thermal")
        assert int(bad.cpu()) == M
    else:
        p, w = EL._points_weights(et, None)
        Nv, dN, wd = LD._iso_tables(et, p, w, torch.device(dev))
        n_ip = dN.shape[0]
        per = 1 if single else n_ip
        out = dict(sig=sentinel(dev, (M + 1) * per, 3, 3), vm=sentinel(dev, (M + 1) * per))
        layout = 0 if single else 1
        if tmode is None:
            C.check(lib.fem_iso_stress(C.ptr(cd), C.ptr(ed), M, NPE[et], C.ptr(ud), E_, NU_, C.ptr(dN), C.ptr(wd),
                                       n_ip, layout, C.ptr(out["sig"]), C.ptr(out["vm"]), st), "fem_iso_stress")
        else:
            C.check(lib.fem_iso_stress_thermal(C.ptr(cd), C.ptr(ed), M, NPE[et], C.ptr(ud), E_, NU_, ALPHA,
                                               C.ptr(Td), tm, T_REF, C.ptr(Nv), C.ptr(dN), C.ptr(wd), n_ip, layout,
                                               C.ptr(out["sig"]), C.ptr(out["vm"]), st), "fem_iso_stress_thermal")
    torch.cuda.synchronize()
    return split_tail(out, M * per)


@pytest.mark.parametrize("et,M", STRESS_CASES)
def test_thermal_stress_at_reference_temperature(gpu, et, M):
    from fem355 import element as EL, loads as LD
    c, el, u = stress_case(et)
    for single in ((True,) if et == "c3d4" else (True, False)):
        plain = stress_launch(gpu, et, M, single)
        assert float(plain["vm"].min()) > 0.0
        more = stress_launch(gpu, et, M + 1, single)
        for k in plain:
            assert torch.equal(more[k][:plain[k].shape[0]], plain[k]), (k, single)
        # the public functions run the same launches
        if et == "c3d4":
            api = EL.compute_c3d4_element_stress(c, el[:M], u, E_, NU_, device=gpu, dtype=F64)
        else:
            api = EL.compute_element_stress(c, el[:M], u, E_, NU_, et, single=single, device=gpu, dtype=F64)
        assert torch.equal(api[0].cpu().reshape(-1, 3, 3), plain["sig"]) and torch.equal(api[1].cpu().reshape(-1),
                                                                                          plain["vm"])
        for tmode in ("uniform", "nodal", "element"):
            th = stress_launch(gpu, et, M, single, tmode)
            if et == "c3d4":
                for k in plain:
                    assert torch.equal(th[k], plain[k]), (k, single, tmode)
            more = stress_launch(gpu, et, M + 1, single, tmode)
            for k in th:
                assert torch.equal(more[k][:th[k].shape[0]], th[k]), (k, single, tmode)
            T = {"uniform": T_REF, "nodal": torch.full((c.shape[0],), T_REF, dtype=F64),
                 "element": torch.full((M,), T_REF, dtype=F64)}[tmode]
            api = LD.compute_thermal_element_stress(c, el[:M], et, u, E_, NU_, ALPHA, T, T_REF, single=single,
                                                    device=gpu, dtype=F64)
            assert torch.equal(api[0].cpu().reshape(-1, 3, 3), th["sig"]), (single, tmode)
            assert torch.equal(api[1].cpu().reshape(-1), th["vm"]), (single, tmode)
