"""CPU fp64 restatement of the penalty contact of the explicit dynamics, written from the formulation on
top of explicit_ref (Model, lumped_mass, element_dt) with plain per-node loops over the surfaces in index order:
    plane     g = (x - c) . n, nu = n
    sphere    r = x - c, g = |r| - R, nu = r / |r|; a cavity: g = R - |r|, nu = -r / |r|
    cylinder  r = (x - c) - ((x - c) . n) n, g and nu as for the sphere
    normal    p = max(0, -g), f_n = k p nu, k = kappa m / dt^2; nothing for |r| = 0, g >= 0 or m = 0
    friction  for the touched surfaces in index order: vt = tangential part of v* - w,
              f_t = -min(mu |f_n|, m |vt| / sigma) vt / |vt|, then v* += sigma f_t / m; v* starts as the half-step
              velocity the update gives with every normal force and no friction, sigma = dt c2 (dt / 2 in the first step)
    held dofs components of f_n and f_t dropped, v* = 0 there
    step      rm = (amp F - f_int + f_c) / m, the leapfrog of explicit_ref.leapfrog otherwise
A surface stands at c + d(t_n) during step n with the velocity (d(t_{n+1}) - d(t_n)) / dt (a constant velocity w:
d = w t and exactly w); the closing evaluation uses the final position and the last step's velocity."""
import math

import torch

F64 = torch.float64


class Surface:
    def __init__(self, kind, point, normal=None, axis=None, radius=None, inside=False, friction=0.0, velocity=None,
                 displacement=None, nodes=None):
        self.kind = kind
        self.point = [float(x) for x in point]
        d = normal if kind == "plane" else axis
        self.n = [0.0, 0.0, 0.0]
        if kind != "sphere":
            ln = math.sqrt(sum(float(x) ** 2 for x in d))
            self.n = [float(x) / ln for x in d]
        self.R = 0.0 if kind == "plane" else float(radius)
        self.inside = bool(inside) and kind != "plane"
        self.mu = float(friction)
        self.velocity = None if velocity is None else [float(x) for x in velocity]
        self.displacement = displacement
        self.nodes = None if nodes is None else set(int(i) for i in nodes)

    def offset(self, t):
        if self.displacement is not None:
            return [float(x) for x in self.displacement(t)]
        if self.velocity is not None:
            return [w * t for w in self.velocity]
        return [0.0, 0.0, 0.0]

    def step_velocity(self, t0, t1):
        if self.displacement is None:
            return list(self.velocity) if self.velocity is not None else [0.0, 0.0, 0.0]
        a, b = self.offset(t0), self.offset(t1)
        return [(y - x) / (t1 - t0) for x, y in zip(a, b)]

    def kwargs(self):
        """The keyword arguments of the same surface as a system.RigidSurface."""
        kw = dict(kind=self.kind, point=self.point, radius=self.R or None, inside=self.inside, friction=self.mu,
                  velocity=self.velocity, displacement=self.displacement,
                  nodes=None if self.nodes is None else sorted(self.nodes))
        kw["normal" if self.kind == "plane" else "axis"] = None if self.kind == "sphere" else self.n
        return kw


def gap(s, c, x):
    """(g, nu) of surface s with its reference point at c, or None where the node has no normal (|r| = 0)."""
    r = [x[q] - c[q] for q in range(3)]
    if s.kind == "plane":
        return sum(r[q] * s.n[q] for q in range(3)), list(s.n)
    if s.kind == "cylinder":
        dn = sum(r[q] * s.n[q] for q in range(3))
        r = [r[q] - dn * s.n[q] for q in range(3)]
    rr = math.sqrt(sum(t * t for t in r))
    if not rr > 0.0:
        return None
    sg = -1.0 if s.inside else 1.0
    return sg * (rr - s.R), [sg * t / rr for t in r]


def contact_forces(surfaces, centres, vels, X, u, m, free, num, vo, dt, kappa, first, alpha):
    """The contact force on every node for the state (u, vo) with num = amp F - f_int: vo is v_n in the first step and
    the half-step velocity otherwise. Returns (f_c [3N] list, per-node records [(i, s, p, nu, fn, ft, vt)], per-surface
    sums [S][reaction 3, count, max penetration], penalty energy)."""
    N = len(m)
    c1, c2 = 1.0 - 0.5 * alpha * dt, 1.0 / (1.0 + 0.5 * alpha * dt)
    sigma = 0.5 * dt if first else dt * c2
    fc = [0.0] * (3 * N)
    recs = []
    per = [[0.0, 0.0, 0.0, 0, 0.0] for _ in surfaces]
    energy = 0.0
    for i in range(N):
        mi = m[i]
        if not mi > 0.0:
            continue
        fr = [bool(free[3 * i + q]) for q in range(3)]
        x = [X[3 * i + q] + (u[3 * i + q] if fr[q] else 0.0) for q in range(3)]
        k = kappa * mi / (dt * dt)
        touched = []
        fn = [0.0, 0.0, 0.0]
        for si, s in enumerate(surfaces):
            if s.nodes is not None and i not in s.nodes:
                continue
            gn = gap(s, centres[si], x)
            if gn is None or not -gn[0] > 0.0:
                continue
            p, nu = -gn[0], gn[1]
            touched.append((si, p, nu))
            for q in range(3):
                fn[q] += k * p * nu[q]
        if not touched:
            continue
        vs = [0.0, 0.0, 0.0]
        for q in range(3):
            if fr[q]:
                rn = (num[3 * i + q] + fn[q]) / mi
                v = vo[3 * i + q]
                vs[q] = v + 0.5 * dt * (rn - alpha * v) if first else (c1 * v + dt * rn) * c2
        for si, p, nu in touched:
            s, w = surfaces[si], vels[si]
            fnm = k * p
            fs = [fnm * nu[q] if fr[q] else 0.0 for q in range(3)]
            rel = [vs[q] - w[q] for q in range(3)]
            vnn = sum(rel[q] * nu[q] for q in range(3))
            vt = [rel[q] - vnn * nu[q] for q in range(3)]
            vtm = math.sqrt(sum(t * t for t in vt))
            ft = [0.0, 0.0, 0.0]
            if s.mu > 0.0 and vtm > 0.0:
                cap = min(s.mu * fnm, mi * vtm / sigma)
                ft = [-cap * vt[q] / vtm if fr[q] else 0.0 for q in range(3)]
                for q in range(3):
                    vs[q] += sigma * ft[q] / mi
                    fs[q] += ft[q]
            for q in range(3):
                fc[3 * i + q] += fs[q]
                per[si][q] -= fs[q]
            per[si][3] += 1
            per[si][4] = max(per[si][4], p)
            energy += 0.5 * k * p * p
            recs.append(dict(node=i, surface=si, p=p, nu=nu, fn=fnm, ft=ft, vt=vt, w=w, fs=fs, mu=s.mu))
    return fc, recs, per, energy


def leapfrog(model, coords, m, free, dt, steps, surfaces, kappa=0.5, F=None, amps=None, u0=None, v0=None, alpha=0.0,
             energy_every=0, contact_every=0, t0=0.0, keep=False):
    """explicit_ref.leapfrog with the contact force. Besides U, V, A and the energy rows: FC [steps + 1, 3N] the contact
    force of every evaluation, and per contact step `reaction` [rows, S, 3], `in_contact` [rows, S], `penetration`
    [rows, S], `min_gap` (see min_abs_gap); per energy step `contact_energy`, `friction_power`, `surface_power`.
    keep: the per-node records of every evaluation in `records` (a list per evaluation)."""
    n = 3 * model.N
    X = coords.to(F64).reshape(-1).tolist()
    ml = m.tolist()
    md = m.repeat_interleave(3)
    free = free & (md > 0)
    fl = free.tolist()
    mi = torch.where(free, 1.0 / md.clamp(min=1e-300), torch.zeros(n, dtype=F64))
    z = lambda: torch.zeros(n, dtype=F64)
    Fv = z() if F is None else F.to(F64).reshape(-1)
    amps = [1.0] * (steps + 1) if amps is None else [float(a) for a in amps]
    u = (z() if u0 is None else u0.to(F64).reshape(-1).clone()) * free
    v = (z() if v0 is None else v0.to(F64).reshape(-1).clone()) * free
    U, V, A, FC = [u.clone()], [], [], []
    en = {k: [] for k in ("t", "kinetic", "strain", "ext_power", "ext_work", "contact_energy", "friction_power",
                          "surface_power")}
    hist = {k: [] for k in ("t_contact", "reaction", "in_contact", "penetration")}
    records = []
    c1, c2 = 1.0 - 0.5 * alpha * dt, 1.0 / (1.0 + 0.5 * alpha * dt)
    vh = None
    for k in range(steps + 1):
        t = t0 + k * dt
        kv = min(k, max(steps - 1, 0))
        centres = [[c + d for c, d in zip(s.point, s.offset(t))] for s in surfaces]
        vels = [s.step_velocity(t0 + kv * dt, t0 + (kv + 1) * dt) for s in surfaces]
        num = amps[k] * Fv - model.f_int(u)
        first = vh is None
        fcl, recs, per, pen_energy = contact_forces(surfaces, centres, vels, X, u.tolist(), ml, fl, num.tolist(),
                                                    (v if first else vh).tolist(), dt, kappa, first, alpha)
        fc = torch.tensor(fcl, dtype=F64)
        rm = (num + fc) * mi
        if first:
            vn = v
            an = (rm - alpha * vn) * free
            vhn = vn + 0.5 * dt * an
        else:
            vhn = (c1 * vh + dt * rm) * c2
            vn = 0.5 * (vh + vhn)
            an = (rm - alpha * vn) * free
        V.append(vn.clone())
        A.append(an.clone())
        FC.append(fc)
        if keep:
            records.append(recs)
        if k == steps:
            break
        if contact_every and k % contact_every == 0:
            hist["t_contact"].append(t)
            hist["reaction"].append([p[:3] for p in per])
            hist["in_contact"].append([p[3] for p in per])
            hist["penetration"].append([p[4] for p in per])
        if energy_every and k % energy_every == 0:
            en["t"].append(k * dt)
            en["kinetic"].append(float(0.5 * (md * vn * vn).sum()))
            en["strain"].append(model.energy(u))
            en["ext_power"].append(float(amps[k] * (Fv @ vn)))
            en["ext_work"].append(float(amps[k] * (Fv @ u)))
            en["contact_energy"].append(pen_energy)
            vl = vn.tolist()
            en["friction_power"].append(sum(r["ft"][q] * (vl[3 * r["node"] + q] - r["w"][q])
                                            for r in recs for q in range(3)))
            en["surface_power"].append(sum(r["fs"][q] * r["w"][q] for r in recs for q in range(3)))
        u = u + dt * vhn
        vh = vhn
        U.append(u.clone())
    S = len(surfaces)
    out = dict(U=torch.stack(U), V=torch.stack(V), A=torch.stack(A), FC=torch.stack(FC), records=records)
    out.update({k: torch.tensor(x, dtype=F64) for k, x in en.items()})
    out["t_contact"] = torch.tensor(hist["t_contact"], dtype=F64)
    out["reaction"] = torch.tensor(hist["reaction"], dtype=F64).reshape(-1, S, 3)
    out["in_contact"] = torch.tensor(hist["in_contact"], dtype=torch.int64).reshape(-1, S)
    out["penetration"] = torch.tensor(hist["penetration"], dtype=F64).reshape(-1, S)
    return out


def min_abs_gap(surfaces, coords, u, t, nodes=None):
    """Per surface the smallest |g| over the nodes at displacement u [3N] and time t: a count may differ between the
    device and the restatement only where this is at rounding level."""
    X = coords.to(F64).reshape(-1, 3)
    x = (X + u.view(-1, 3)).tolist()
    out = []
    for s in surfaces:
        c = [a + b for a, b in zip(s.point, s.offset(t))]
        best = math.inf
        for i, xi in enumerate(x):
            if s.nodes is not None and i not in s.nodes:
                continue
            gn = gap(s, c, xi)
            if gn is not None:
                best = min(best, abs(gn[0]))
        out.append(best)
    return out
