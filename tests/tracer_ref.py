"""NumPy float64 replay of the massless tracers (include/nbmi.h nbmi_set_tracers): both integrators in
the association the header writes, per component, without FMA (NumPy rounds every product and every sum).

The field is a callable ``force(points) -> acc`` over (k, 3) arrays.  A substep of the bodies lies between ``begin``
and ``end``: ``begin`` gets the field of the bodies before it, ``end`` the field of the bodies after it, which is what the
leapfrog's closing half-kick uses.  ``step`` is both with one field (a potential that does not move)."""
import numpy as np

LIMIT = 1e18  # a tracer beyond it in any coordinate is retired, as nbmi_field_at refuses such a point


class TracerReplay:
    def __init__(self, positions, velocities=None, integrator="kick_drift", damping=1.0):
        if integrator not in ("kick_drift", "leapfrog"):
            raise ValueError(integrator)
        self.p = np.array(positions, dtype=np.float64)
        self.v = np.zeros_like(self.p) if velocities is None else np.array(velocities, dtype=np.float64)
        self.a = None  # leapfrog: a = F(p) of the current state; None: the next begin primes it
        self.integrator, self.damping = integrator, float(damping)

    def drop_acceleration(self):
        """what nbmi_set_state, a switch of integrator or multipole and a reported capacity error do"""
        self.a = None

    def _live(self, with_a):
        ok = np.all(np.abs(self.p) <= LIMIT, axis=1) & np.all(np.isfinite(self.v), axis=1)
        if with_a:
            ok &= np.all(np.isfinite(self.a), axis=1)
        return ok

    def _field(self, force, live):
        a = np.zeros_like(self.p)
        if live.any():
            a[live] = np.asarray(force(np.ascontiguousarray(self.p[live])), dtype=np.float64)
        return a

    def begin(self, dt, force):
        p, v = self.p, self.v
        if self.integrator == "kick_drift":
            live = self._live(False)
            a = self._field(force, live)
            v[live] = ((v + a * dt) * self.damping)[live]
            p[live] = (p + v * dt)[live]
            return
        h = 0.5 * dt
        if self.a is None:  # the priming walk: a stored, state untouched
            self.a = self._field(force, self._live(False))
        live = self._live(True)
        v[live] = (v + self.a * h)[live]
        p[live] = (p + v * dt)[live]

    def end(self, dt, force):
        if self.integrator == "kick_drift":
            return
        h = 0.5 * dt
        live = self._live(False)
        a = self._field(force, live)
        self.a[live] = a[live]
        self.v[live] = ((self.v + a * h) * self.damping)[live]

    def step(self, dt, force):
        self.begin(dt, force)
        self.end(dt, force)


def point_mass_field(center, gm, eps=0.0):
    """force(points) of one body of G m = ``gm`` at ``center`` as the header's term: d = c - p, dist_sq = ((dx dx + dy dy)
    + dz dz) + eps^2, applied where dist_sq > eps^2, acc = d * (G M / (dist * dist_sq)) - the bits of a one-body handle."""
    c = np.asarray(center, dtype=np.float64).reshape(3)
    e2 = float(eps) * float(eps)

    def force(points):
        d = c[None, :] - np.asarray(points, dtype=np.float64)
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + e2
        on = d2 > e2
        w = np.zeros(len(d))
        w[on] = gm / (np.sqrt(d2[on]) * d2[on])
        return 0.0 + d * w[:, None]  # (the kernel's sum starts at +0.0)
    return force
