"""ctypes view of libdedflow.so (the C host layer + HIP kernels) for the Python
harness (tests, bench.py, __graft_entry__).  Python never computes anything on
the path: it generates synthetic inputs, calls the C object API in the order of
the reference driver (``src/main.c:372-477``) and copies results back.

The library is the product; if it is missing, importing this module's
``lib()`` raises -- there is no CPU or PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_HIP = None

c_i32p = C.POINTER(C.c_int32)
c_f64p = C.POINTER(C.c_double)
vp = C.c_void_p


class MissingExtension(RuntimeError):
    pass


def lib_path() -> str:
    # DFL_LIB: an alternative build of the same library (`make asan`: host layer under AddressSanitizer / UBSan, CPU runs only)
    return os.environ.get("DFL_LIB") or os.path.join(_HERE, "libdedflow.so")


def lib():
    """Load libdedflow.so; fail loudly (no fallback) when it has not been built."""
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise MissingExtension(
                f"{p} not found: build it with `make` (or __graft_entry__.build()); the hot path has no CPU fallback")
        L = C.CDLL(p, mode=C.RTLD_GLOBAL)
        _declare(L)
        _LIB = L
    return _LIB


def hip():
    global _HIP
    if _HIP is None:
        H = C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
        H.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
        H.hipFree.argtypes = [vp]
        H.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
        H.hipMemset.argtypes = [vp, C.c_int, C.c_size_t]
        H.hipDeviceSynchronize.argtypes = []
        H.hipEventCreate.argtypes = [C.POINTER(vp)]
        H.hipEventRecord.argtypes = [vp, vp]
        H.hipEventSynchronize.argtypes = [vp]
        H.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
        H.hipEventDestroy.argtypes = [vp]
        H.hipGetErrorString.restype = C.c_char_p
        H.hipSetDevice.argtypes = [C.c_int]
        _HIP = H
    return _HIP


def _chk(e):
    if e != 0:
        raise RuntimeError("HIP error %d: %s" % (e, hip().hipGetErrorString(e).decode()))


H2D, D2H, D2D = 1, 2, 3


class DeviceArray:
    """Raw device buffer (hipMalloc, zero-filled) with numpy transfer helpers."""

    def __init__(self, n, dtype=np.float64, ptr=None, owner=True):
        self.dtype = np.dtype(dtype)
        self.n = int(n)
        self.nbytes = self.n * self.dtype.itemsize
        self.owner = owner and ptr is None
        if ptr is None:
            p = vp()
            _chk(hip().hipMalloc(C.byref(p), max(self.nbytes, 16)))
            _chk(hip().hipMemset(p, 0, max(self.nbytes, 16)))
            self.ptr = p.value
        else:
            self.ptr = int(ptr)

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a)
        d = cls(a.size, a.dtype)
        d.upload(a)
        return d

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.size == self.n
        _chk(hip().hipMemcpy(self.ptr, a.ctypes.data, self.nbytes, H2D))

    def numpy(self):
        out = np.empty(self.n, self.dtype)
        if self.nbytes:
            _chk(hip().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, D2H))
        return out

    def zero(self):
        _chk(hip().hipMemset(self.ptr, 0, max(self.nbytes, 1)))

    def view(self, offset, n):
        return DeviceArray(n, self.dtype, ptr=self.ptr + offset * self.dtype.itemsize)

    def free(self):
        if self.owner and self.ptr:
            hip().hipFree(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def d2h(ptr, n, dtype):
    return DeviceArray(n, dtype, ptr=ptr).numpy()


def sync():
    _chk(hip().hipDeviceSynchronize())


class Timer:
    """hipEvent pair on the library stream (the null stream unless DflSetStream was called)."""

    def __init__(self):
        self.a, self.b = vp(), vp()
        _chk(hip().hipEventCreate(C.byref(self.a)))
        _chk(hip().hipEventCreate(C.byref(self.b)))

    def start(self):
        _chk(hip().hipEventRecord(self.a, lib().DflStream()))

    def stop(self):
        _chk(hip().hipEventRecord(self.b, lib().DflStream()))

    def ms(self):
        _chk(hip().hipEventSynchronize(self.b))
        t = C.c_float(0)
        _chk(hip().hipEventElapsedTime(C.byref(t), self.a, self.b))
        return float(t.value)


# ---- struct mirrors of include/dedflow.h ---------------------------------------------
class Mesh3DData(C.Structure):
    _fields_ = [("is_host", C.c_int32), ("num_node", C.c_int32), ("num_tet", C.c_int32), ("num_prism", C.c_int32),
                ("num_hex", C.c_int32), ("xg", vp), ("ien", vp)]


class Mesh3D(C.Structure):
    _fields_ = [("num_node", C.c_int32), ("num_tet", C.c_int32), ("num_prism", C.c_int32), ("num_hex", C.c_int32),
                ("host", C.POINTER(Mesh3DData)), ("device", C.POINTER(Mesh3DData)),
                ("num_bound", C.c_int32), ("bound_fid", vp), ("bound_node_offset", vp), ("bound_node", vp),
                ("bound_elem_offset", vp), ("bound_ien", vp), ("bound_f2e", vp), ("bound_forn", vp),
                ("num_batch", C.c_int32), ("batch_offset", vp), ("batch_ind", vp),
                ("num_color", C.c_int32), ("color", vp), ("ext", vp)]


class CSRAttr(C.Structure):
    pass


CSRAttr._fields_ = [("num_row", C.c_int32), ("num_col", C.c_int32), ("nnz", C.c_int32), ("row_ptr", vp), ("col_ind", vp),
                    ("parent", C.POINTER(CSRAttr)), ("diag_pos", vp)]


class Matrix(C.Structure):
    _fields_ = [("size", C.c_int32 * 2), ("type", C.c_int), ("data", vp), ("stream_ref", vp), ("op", vp * 15)]


class MatrixCSR(C.Structure):
    _fields_ = [("external_attr", C.c_int32), ("attr", C.POINTER(CSRAttr)), ("val", vp), ("descr", vp),
                ("buffer_size", C.c_int32), ("buffer", vp), ("owner", vp), ("owner_slot", C.c_int32)]


class MatrixFS(C.Structure):
    _fields_ = [("n_offset", C.c_int32), ("offset", vp), ("d_offset", vp), ("stream", vp), ("spy1x1", C.POINTER(CSRAttr)),
                ("d_matval", vp), ("mat", C.POINTER(C.POINTER(Matrix))), ("block_mode", C.c_int32), ("block_val", vp)]


class KrylovStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("rnrm_init", C.c_double), ("res_hist", C.c_double * 512), ("converged", C.c_int32),
                ("fused_norm_cancelled", C.c_int32), ("total_solves", C.c_int32), ("total_converged", C.c_int32),
                ("total_iterations", C.c_int64)]


class Dirichlet(C.Structure):
    _fields_ = [("mesh", vp), ("face_ind", C.c_int32), ("shape", C.c_int32), ("buffer_size", C.c_size_t), ("buffer", vp)]
    # followed by BCType bctype[shape]


class Array(C.Structure):
    _fields_ = [("is_host", C.c_int32), ("len", C.c_int32), ("data", vp)]


class ParticleContext(C.Structure):
    _fields_ = [("num_particle", C.c_int32), ("num_pointwise_dof", C.c_int32), ("h_arr", C.POINTER(Array) * 3),
                ("d_arr", C.POINTER(Array) * 3), ("buff", C.c_double * 2), ("ext", vp)]


class Particles:
    """ParticleContext (src/Particle.h) + the build-defined contact sweep."""

    def __init__(self, coord, vel, radius, mass=1.0, kn=1.0e4, gamma_n=1.0, dt=1.0e-4):
        L = lib()
        L.Init(0, None)
        P = coord.size // 3
        self.ctx = L.ParticleContextCreate(P)
        c = self.ctx.contents
        c.buff[0], c.buff[1] = mass, radius
        C.memmove(c.h_arr[0].contents.data, np.ascontiguousarray(coord).ctypes.data, 24 * P)
        C.memmove(c.h_arr[1].contents.data, np.ascontiguousarray(vel).ctypes.data, 24 * P)
        L.ParticleContextUpdateDevice(self.ctx)
        L.ParticleContextSetContactModel(self.ctx, kn, gamma_n, dt)

    @property
    def P(self):
        """the current particle count (changes under add() / remove())"""
        return int(self.ctx.contents.num_particle)

    def compute_forces(self):
        lib().ParticleContextComputeForces(self.ctx)

    def update(self):
        lib().ParticleContextUpdate(self.ctx)

    # ---- particle-fluid coupling (build-defined; model in include/dedflow.h) --------------------------------------
    def couple(self, problem, rho_f=1e3, mu_f=10.0 / 3.0, gravity=(0.0, 0.0, 0.0), two_way=False):
        """ParticleContextSetFluidCoupling with problem's mesh; problem None turns the coupling off."""
        if problem is None:
            lib().ParticleContextSetFluidCoupling(self.ctx, None, None)
            self.N = 0
            return
        cfg = DflFluidCoupling(rho_f, mu_f, (C.c_double * 3)(*gravity), 1 if two_way else 0)
        lib().ParticleContextSetFluidCoupling(self.ctx, problem.mesh, C.byref(cfg))
        self.N = problem.N

    def locate(self):
        lib().ParticleContextLocate(self.ctx)

    def tet(self):
        """tet of every particle (-1 outside the mesh, -2 walk cap hit)"""
        return d2h(lib().ParticleContextTet(self.ctx), self.P, np.int32)

    def barycentric(self):
        return d2h(lib().ParticleContextBarycentric(self.ctx), 4 * self.P, np.float64).reshape(self.P, 4)

    def lost_count(self):
        return int(lib().ParticleContextLostCount(self.ctx))

    def fluid_step(self, w):
        """one coupled sub-step in the fluid state w (DeviceArray of 6N)"""
        lib().ParticleContextFluidStep(self.ctx, w.ptr)

    def reaction_load(self, out=None):
        """ParticleContextReactionLoad into `out` (DeviceArray of 3N, allocated when None); returns the DeviceArray"""
        if out is None:
            out = DeviceArray(3 * self.N)
        lib().ParticleContextReactionLoad(self.ctx, out.ptr)
        return out

    # ---- walls from a mesh's boundary faces (build-defined; model in include/dedflow.h) ----------------------------
    def set_walls(self, problem, groups=range(6)):
        """ParticleContextSetWallMesh: the boundary faces of `groups` of problem's mesh become the walls (the other groups
        are open); problem None returns to the unit box."""
        if problem is None:
            lib().ParticleContextSetWallMesh(self.ctx, None, 0)
            return
        mask = 0
        for g in groups:
            mask |= 1 << int(g)
        lib().ParticleContextSetWallMesh(self.ctx, problem.mesh, mask)

    def wall_dropped_count(self):
        return int(lib().ParticleContextWallDroppedCount(self.ctx))

    # ---- contact friction and rotation (build-defined; model in include/dedflow.h) --------------------------------
    def set_friction(self, mu, kt=None, gamma_t=None):
        """ParticleContextSetFriction: Coulomb coefficient mu, tangential stiffness kt (None: 2/7 kn) and damping gamma_t
        (None: gamma_n); mu None turns friction off.  Turning it on starts every particle at zero spin; later calls keep
        the spin and clear the contact history."""
        if mu is None:
            lib().ParticleContextSetFriction(self.ctx, None)
            return
        cfg = DflContactFriction(float(mu), 0.0 if kt is None else float(kt), -1.0 if gamma_t is None else float(gamma_t))
        lib().ParticleContextSetFriction(self.ctx, C.byref(cfg))

    def set_gravity(self, g):
        """body acceleration g[3] of update() (not of fluid_step, which uses the coupling's gravity)"""
        lib().ParticleContextSetGravity(self.ctx, (C.c_double * 3)(*[float(a) for a in g]))

    def _spin_ptr(self, name):
        p = getattr(lib(), name)(self.ctx)
        if not p:
            raise RuntimeError("friction is off: call set_friction first")
        return p

    def omega(self):
        """angular velocity [P][3] copied back from the device"""
        return d2h(self._spin_ptr("ParticleContextAngularVelocity"), 3 * self.P, np.float64).reshape(self.P, 3)

    def set_omega(self, w):
        """overwrite the angular velocity with w ([P][3])"""
        p = self._spin_ptr("ParticleContextAngularVelocity")
        sync()
        DeviceArray(3 * self.P, ptr=p).upload(np.asarray(w, dtype=np.float64).reshape(-1))

    def alpha(self):
        """angular acceleration (torque / I) [P][3] of the last contact sweep"""
        return d2h(self._spin_ptr("ParticleContextAngularAcc"), 3 * self.P, np.float64).reshape(self.P, 3)

    def friction_history(self):
        """the contact history the next sweep reads: keys [P][16] uint64, springs xi [P][16][3], live counts [P]"""
        rows, counts = vp(), C.POINTER(C.c_int32)()
        lib().ParticleContextFrictionHistory(self.ctx, C.byref(rows), C.byref(counts))
        if not rows.value:
            raise RuntimeError("friction is off: call set_friction first")
        raw = d2h(rows.value, 4 * 16 * self.P, np.float64).reshape(self.P, 16, 4)
        keys = raw[:, :, 0].copy().view(np.uint64)
        return keys, raw[:, :, 1:].copy(), d2h(C.cast(counts, vp).value, self.P, np.int32)

    def friction_overflow_count(self):
        return int(lib().ParticleContextFrictionOverflowCount(self.ctx))

    # ---- particle inflow and outflow (build-defined; model in include/dedflow.h) ------------------------------------
    def set_outflow(self, planes=(), outside_mesh=False):
        """ParticleContextSetOutflow: remove() drops the particles with n . x > d for any (n0, n1, n2, d) in `planes` and, with
        outside_mesh on a coupled context, those located outside the mesh; planes None turns outflow off"""
        if planes is None:
            lib().ParticleContextSetOutflow(self.ctx, None)
            return
        planes = np.asarray(planes, dtype=np.float64).reshape(-1, 4)
        if len(planes) > DFL_OUTFLOW_MAX_PLANES:
            raise ValueError(f"at most {DFL_OUTFLOW_MAX_PLANES} outflow planes")
        cfg = DflParticleOutflow()
        cfg.num_planes = len(planes)
        for k, pl in enumerate(planes):
            for d in range(4):
                cfg.plane[k][d] = float(pl[d])
        cfg.outside_mesh = 1 if outside_mesh else 0
        lib().ParticleContextSetOutflow(self.ctx, C.byref(cfg))

    def set_inflow(self, origin, edge_u, edge_v, vel=(0.0, 0.0, 0.0), per_call=1.0, jitter=0.0, seed=0, max_particles=2**31 - 1):
        """ParticleContextSetInflow: add() inserts into the slots of the inlet rectangle origin + s edge_u + t edge_v;
        origin None turns inflow off"""
        if origin is None:
            lib().ParticleContextSetInflow(self.ctx, None)
            return
        v3 = lambda a: (C.c_double * 3)(*[float(q) for q in a])
        cfg = DflParticleInflow(v3(origin), v3(edge_u), v3(edge_v), v3(vel), float(per_call), float(jitter), int(seed),
                                int(max_particles))
        lib().ParticleContextSetInflow(self.ctx, C.byref(cfg))

    def add(self):
        lib().ParticleContextAdd(self.ctx)

    def remove(self):
        lib().ParticleContextRemove(self.ctx)

    def tags(self):
        """stable 64-bit tag of every particle (None until inflow or outflow was set)"""
        p = lib().ParticleContextTag(self.ctx)
        return None if not p else d2h(p, self.P, np.int64)

    def flow_stats(self):
        """dict inserted / removed / blocked since the first set_inflow / set_outflow"""
        st = DflParticleFlowStats()
        lib().ParticleContextFlowStats(self.ctx, C.byref(st))
        return {"inserted": int(st.inserted), "removed": int(st.removed), "blocked": int(st.blocked)}

    # ---- polydisperse particles (build-defined; model in include/dedflow.h) ------------------------------------------
    def set_sizes(self, radius, mass=None):
        """ParticleContextSetSizes: per-particle radius [P] and mass [P] (None: the reference particle's density,
        m = mass (r / radius)^3); radius None returns to monodisperse.  Raises ValueError on a non-positive or non-finite
        value (the context is left unchanged)"""
        if radius is None:
            lib().ParticleContextSetSizes(self.ctx, None, None)
            return
        r = np.ascontiguousarray(radius, dtype=np.float64).reshape(-1)
        m = None if mass is None else np.ascontiguousarray(mass, dtype=np.float64).reshape(-1)
        if r.size != self.P or (m is not None and m.size != self.P):
            raise ValueError(f"set_sizes: need {self.P} radii (and masses)")
        if not (np.all(np.isfinite(r)) and np.all(r > 0) and (m is None or (np.all(np.isfinite(m)) and np.all(m > 0)))):
            raise ValueError("set_sizes: radii and masses must be positive and finite")
        lib().ParticleContextSetSizes(self.ctx, r.ctypes.data, None if m is None else m.ctypes.data)

    def radii(self):
        """radius of every particle [P] (None when monodisperse)"""
        p = lib().ParticleContextRadii(self.ctx)
        return None if not p else d2h(p, self.P, np.float64)

    def masses(self):
        """mass of every particle [P] (None when monodisperse)"""
        p = lib().ParticleContextMasses(self.ctx)
        return None if not p else d2h(p, self.P, np.float64)

    @property
    def max_radius(self):
        """Rmax: the bound on every radius the grids are built for (the radius when monodisperse)"""
        return float(lib().ParticleContextMaxRadius(self.ctx))

    def set_inflow_sizes(self, r_lo, r_hi):
        """ParticleContextSetInflowSizes: add() inserts radii in [r_lo, r_hi) (makes the context polydisperse)"""
        if not (0.0 < float(r_lo) <= float(r_hi) and np.isfinite(r_hi)):
            raise ValueError("set_inflow_sizes: need 0 < r_lo <= r_hi")
        lib().ParticleContextSetInflowSizes(self.ctx, float(r_lo), float(r_hi))

    # ---- particle heat transfer (build-defined; model in include/dedflow.h) -----------------------------------------
    def set_heat(self, cp_p, k_p=0.0, cp_f=0.0, k_f=0.0, T_init=0.0, two_way=False):
        """ParticleContextSetHeat: particle specific heat cp_p (> 0), conductivity k_p (<= 0: no contact conduction), fluid
        cp_f / k_f (<= 0: the reference's constants), the temperature T_init of every particle now and of inserted ones;
        cp_p None turns heat off."""
        if cp_p is None:
            lib().ParticleContextSetHeat(self.ctx, None)
            return
        if not (float(cp_p) > 0.0 and np.isfinite(cp_p) and np.isfinite(T_init)):
            raise ValueError("set_heat: need cp_p > 0 and a finite T_init")
        cfg = DflParticleHeat(float(cp_p), float(k_p), float(cp_f), float(k_f), float(T_init), 1 if two_way else 0)
        lib().ParticleContextSetHeat(self.ctx, C.byref(cfg))

    def _heat_ptr(self, name):
        p = getattr(lib(), name)(self.ctx)
        if not p:
            raise RuntimeError("heat is off: call set_heat first")
        return p

    def temperature(self):
        """temperature of every particle [P] copied back from the device"""
        return d2h(self._heat_ptr("ParticleContextTemperature"), self.P, np.float64)

    def set_temperature(self, T):
        """overwrite the particle temperatures with T ([P])"""
        p = self._heat_ptr("ParticleContextTemperature")
        sync()
        DeviceArray(self.P, ptr=p).upload(np.asarray(T, dtype=np.float64).reshape(-1))

    def heat_rate(self):
        """heat flowing into every particle [P] in the last heat step"""
        return d2h(self._heat_ptr("ParticleContextHeatRate"), self.P, np.float64)

    def _pending_energy(self):
        """energy the fluid gave every particle [P] since the last heat_source (library-private accessor, for tests)"""
        return d2h(self._heat_ptr("DflParticlePendingEnergy"), self.P, np.float64)

    def _conduction_rate(self):
        """q_i [P] of the last heat step with k_p > 0 (library-private accessor, for tests)"""
        return d2h(self._heat_ptr("DflParticleConductionRate"), self.P, np.float64)

    def heat_step(self, w=None):
        """ParticleContextHeatStep: one thermal sub-step in the fluid state w (DeviceArray of 6N; None: conduction only)"""
        self._heat_ptr("ParticleContextTemperature")
        lib().ParticleContextHeatStep(self.ctx, w.ptr if w is not None else None)

    def heat_source(self, out=None):
        """ParticleContextHeatSource into `out` (DeviceArray of N, allocated when None); returns the DeviceArray"""
        self._heat_ptr("ParticleContextTemperature")
        if not getattr(self, "N", 0):
            raise RuntimeError("heat_source needs a coupled context: call couple first")
        if out is None:
            out = DeviceArray(self.N)
        lib().ParticleContextHeatSource(self.ctx, out.ptr)
        return out

    # ---- laser energy deposition (build-defined; model in include/dedflow.h) ----------------------------------------
    def set_laser(self, origin, direction=(0.0, 0.0, -1.0), power=0.0, w=1.0, h=1.0, r_cut=1.0, eta_p=1.0, eta_s=1.0,
                  scan_vel=(0.0, 0.0, 0.0), substrate_groups=()):
        """ParticleContextSetLaser: a collimated Gaussian beam through `origin` along `direction`, power (W), 1/e^2 radius w,
        column edge h and cut-off radius r_cut of the column grid, absorptivities of powder and substrate, the axis'
        velocity, and the boundary groups of the coupled mesh that receive the transmitted beam; origin None turns the
        laser off.  Needs set_heat.  A configuration the library refuses (reported on stderr) leaves the context as it was:
        laser_on tells."""
        if origin is None:
            lib().ParticleContextSetLaser(self.ctx, None)
            return
        mask = 0
        for g in substrate_groups:
            mask |= 1 << int(g)
        v3 = lambda a: (C.c_double * 3)(*[float(q) for q in a])
        cfg = DflLaser(v3(origin), v3(direction), v3(scan_vel), float(power), float(w), float(h), float(r_cut), float(eta_p),
                       float(eta_s), mask)
        lib().ParticleContextSetLaser(self.ctx, C.byref(cfg))

    @property
    def laser_on(self):
        return bool(lib().ParticleContextLaserRate(self.ctx))

    def _laser_ptr(self):
        p = lib().ParticleContextLaserRate(self.ctx)
        if not p:
            raise RuntimeError("the laser is off: call set_laser first")
        return p

    def laser_step(self, dt):
        """ParticleContextLaserStep: bin, attenuation, deposit and tally with the beam advanced by dt; no temperature update"""
        self._laser_ptr()
        lib().ParticleContextLaserStep(self.ctx, float(dt))

    def laser_rate(self):
        """W absorbed by every particle [P] in the last laser step"""
        return d2h(self._laser_ptr(), self.P, np.float64)

    def laser_tally(self):
        """dict outside / absorbed_particles / scattered / substrate / reflected / missed of the last laser step (W)"""
        t = DflLaserTally()
        lib().ParticleContextLaserTally(self.ctx, C.byref(t))
        return {k: float(getattr(t, k)) for k, _ in DflLaserTally._fields_}

    def laser_columns(self):
        """(transmitted power [n n], hit face record id [n n], -1: none) of the last laser step"""
        self._laser_ptr()
        tp, fp = vp(), vp()
        n = int(lib().ParticleContextLaserColumns(self.ctx, C.byref(tp), C.byref(fp)))
        return d2h(tp.value, n, np.float64), d2h(fp.value, n, np.int32)

    # ---- laser on the level-set surface (build-defined; model in include/dedflow.h) ---------------------------------
    def set_laser_surface(self, level=0.0, side=1):
        """ParticleContextSetLaserSurface: the transmitted beam is also deposited on the surface phi = level of the coupled
        mesh (metal where side (phi - level) > 0); level None turns it off.  Needs set_laser and couple.  A configuration the
        library refuses (reported on stderr) leaves the context as it was: laser_surface_on tells."""
        if level is None:
            lib().ParticleContextSetLaserSurface(self.ctx, None)
            return
        cfg = DflLaserSurface(float(level), int(side))
        lib().ParticleContextSetLaserSurface(self.ctx, C.byref(cfg))

    @property
    def laser_surface_on(self):
        return int(lib().ParticleContextLaserSurfaceFacets(self.ctx, None, None)) >= 0

    def laser_surface_update(self, w):
        """ParticleContextLaserSurfaceUpdate at the fluid state w (DeviceArray of 6N): the number of candidate facets, -1 off"""
        return int(lib().ParticleContextLaserSurfaceUpdate(self.ctx, w.ptr))

    def laser_surface_facets(self):
        """(facets [nf, 9], tet [nf]) of the last snapshot, copied back from the device"""
        fp, tp = vp(), vp()
        n = int(lib().ParticleContextLaserSurfaceFacets(self.ctx, C.byref(fp), C.byref(tp)))
        if n < 0:
            raise RuntimeError("no laser surface is set: call set_laser_surface first")
        if n == 0:
            return np.zeros((0, 9)), np.zeros(0, np.int32)
        sync()
        return d2h(fp.value, 9 * n, np.float64).reshape(n, 9), d2h(tp.value, n, np.int32)

    def laser_surface_power(self, out=None):
        """ParticleContextLaserSurfacePower into `out` (DeviceArray of N, allocated when None); returns the DeviceArray"""
        if not self.laser_surface_on:
            raise RuntimeError("no laser surface is set: call set_laser_surface first")
        if out is None:
            out = DeviceArray(self.N)
        lib().ParticleContextLaserSurfacePower(self.ctx, out.ptr)
        return out

    # ---- laser reflections (build-defined; model in include/dedflow.h) ----------------------------------------------
    def set_laser_reflection(self, max_bounce=4, model=1, eps=0.25):
        """ParticleContextSetLaserReflection: column rays that hit a facet of phi = level are reflected up to max_bounce times
        over all its facets, absorbing eta_s (model 0) or a Fresnel share with the material constant eps (model 1) at every
        hit; max_bounce None turns it off.  Needs set_laser and set_laser_surface; the next laser_surface_update takes the
        snapshot the rays run on.  A configuration the library refuses (reported on stderr) leaves the context as it was:
        laser_reflection_on tells."""
        if max_bounce is None:
            lib().ParticleContextSetLaserReflection(self.ctx, None)
            return
        cfg = DflLaserReflection(int(max_bounce), int(model), float(eps))
        lib().ParticleContextSetLaserReflection(self.ctx, C.byref(cfg))

    @property
    def laser_reflection_on(self):
        return int(lib().ParticleContextLaserReflectionFacets(self.ctx, None, None, None)) >= 0

    def laser_reflection_tally(self):
        """dict absorbed [9] / escaped / remaining (W) / rays [9] of the last laser step; zeros when off"""
        t = DflLaserReflectionTally()
        lib().ParticleContextLaserReflectionTally(self.ctx, C.byref(t))
        return dict(absorbed=np.array(t.absorbed[:], np.float64), escaped=float(t.escaped), remaining=float(t.remaining),
                    rays=np.array(t.rays[:], np.int64))

    def laser_reflection_rays(self):
        """(facet [max_bounce + 1, n n] as indices into the reflection list, -1: none; absorbed [max_bounce + 1, n n] in W) of
        the last laser step, copied back from the device; (None, None) before the first step with a reflection list"""
        fp, ap = vp(), vp()
        n = int(lib().ParticleContextLaserReflectionRays(self.ctx, C.byref(fp), C.byref(ap)))
        if n <= 0:
            return None, None
        sync()
        ncol = int(lib().ParticleContextLaserColumns(self.ctx, C.byref(vp()), C.byref(vp())))
        return d2h(fp.value, n, np.int32).reshape(-1, ncol), d2h(ap.value, n, np.float64).reshape(-1, ncol)

    def laser_reflection_facets(self):
        """(facets [nr, 9], tet [nr], gradient [nr, 3]) of the reflection list of the last snapshot, copied back"""
        fp, tp, gp = vp(), vp(), vp()
        n = int(lib().ParticleContextLaserReflectionFacets(self.ctx, C.byref(fp), C.byref(tp), C.byref(gp)))
        if n < 0:
            raise RuntimeError("no laser reflection is set: call set_laser_reflection first")
        if n == 0:
            return np.zeros((0, 9)), np.zeros(0, np.int32), np.zeros((0, 3))
        sync()
        return (d2h(fp.value, 9 * n, np.float64).reshape(n, 9), d2h(tp.value, n, np.int32),
                d2h(gp.value, 3 * n, np.float64).reshape(n, 3))

    # ---- melt-pool capture (build-defined; model in include/dedflow.h) ----------------------------------------------
    def set_capture(self, level=0.0, side=1, reach=0.0, T_melt=-np.inf, two_way=False):
        """ParticleContextSetCapture: capture() takes out the particles that reach the metal surface phi = level (side +1:
        metal where phi > level, -1: where phi < level; reach in particle radii) where the fluid has T_f >= T_melt, and
        deposits their mass, excess momentum and excess heat on the nodes; level None turns capture off.  Needs couple.  A
        configuration the library refuses (reported on stderr) leaves the context as it was: capture_on tells."""
        if level is None:
            lib().ParticleContextSetCapture(self.ctx, None)
            return
        cfg = DflParticleCapture(float(level), int(side), float(reach), float(T_melt), 1 if two_way else 0)
        lib().ParticleContextSetCapture(self.ctx, C.byref(cfg))

    @property
    def capture_on(self):
        return bool(lib().DflParticleCaptureOn(self.ctx))

    def capture(self, w):
        """ParticleContextCapture in the fluid state w (DeviceArray of 6N); returns the number of particles captured"""
        return int(lib().ParticleContextCapture(self.ctx, w.ptr))

    def capture_source(self, time):
        """ParticleContextCaptureSource over the window `time` (> 0): (q_vol [N], load [3N], q_heat [N]) as DeviceArrays; clears
        what was pending"""
        if not self.capture_on:
            raise RuntimeError("capture is off: call set_capture first")
        if not float(time) > 0.0:
            raise ValueError("capture_source: the time window must be positive")
        out = DeviceArray(self.N), DeviceArray(3 * self.N), DeviceArray(self.N)
        lib().ParticleContextCaptureSource(self.ctx, float(time), out[0].ptr, out[1].ptr, out[2].ptr)
        return out

    def capture_stats(self):
        """dict captured (since capture was set) / last (by the last capture call)"""
        st = DflParticleCaptureStats()
        lib().ParticleContextCaptureStats(self.ctx, C.byref(st))
        return {"captured": int(st.captured), "last": int(st.last)}

    # ---- solid-surface contact (build-defined; model in include/dedflow.h) -----------------------------------------
    def set_surface_contact(self, level=0.0, side=1, T_solid=np.inf):
        """ParticleContextSetSurfaceContact: every fluid_step also collides the particles with the surface phi = level (side
        +1: metal where phi > level, -1: where phi < level) wherever the fluid has T_f < T_solid (inf: everywhere); level None
        turns it off.  Needs couple.  A configuration the library refuses (reported on stderr) leaves the context as it was:
        surface_contact_on tells."""
        if level is None:
            lib().ParticleContextSetSurfaceContact(self.ctx, None)
            return
        cfg = DflSurfaceContact(float(level), int(side), float(T_solid))
        lib().ParticleContextSetSurfaceContact(self.ctx, C.byref(cfg))

    @property
    def surface_contact_on(self):
        return bool(lib().DflParticleSurfaceContactOn(self.ctx))

    def surface_contact_stats(self):
        """dict last / buried (particles in contact / buried in the last sub-step) / total (particle-sub-steps in contact
        since the configuration was set); waits for the device"""
        st = DflSurfaceContactStats()
        lib().ParticleContextSurfaceContactStats(self.ctx, C.byref(st))
        return {"last": int(st.last), "buried": int(st.buried), "total": int(st.total)}

    def _surface_contact_apply(self, w):
        """the contact alone, as fluid_step runs it after compute_forces() and locate() (library-private, for tests)"""
        lib().DflSurfaceContactApply(self.ctx, w.ptr)

    def _surface_contact_no_early_exit(self):
        """zero the bound behind the contact kernel's early exit (library-private, for the cost probe; same results)"""
        lib().DflSurfaceContactTestNoEarlyExit(self.ctx)

    def arrays(self):
        """(coord, vel, acc) copied back from the device"""
        c = self.ctx.contents
        return tuple(d2h(c.d_arr[k].contents.data, 3 * self.P, np.float64) for k in range(3))

    def close(self):
        lib().ParticleContextDestroy(self.ctx)


class DflContactFriction(C.Structure):
    _fields_ = [("mu", C.c_double), ("kt", C.c_double), ("gamma_t", C.c_double)]


DFL_OUTFLOW_MAX_PLANES = 8


class DflParticleOutflow(C.Structure):
    _fields_ = [("num_planes", C.c_int32), ("plane", (C.c_double * 4) * DFL_OUTFLOW_MAX_PLANES), ("outside_mesh", C.c_int32)]


class DflParticleInflow(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("edge_u", C.c_double * 3), ("edge_v", C.c_double * 3), ("vel", C.c_double * 3),
                ("per_call", C.c_double), ("jitter", C.c_double), ("seed", C.c_uint64), ("max_particles", C.c_int32)]


class DflParticleFlowStats(C.Structure):
    _fields_ = [("inserted", C.c_int64), ("removed", C.c_int64), ("blocked", C.c_int64)]


class DflParticleHeat(C.Structure):
    _fields_ = [("cp_p", C.c_double), ("k_p", C.c_double), ("cp_f", C.c_double), ("k_f", C.c_double), ("T_init", C.c_double),
                ("two_way", C.c_int32)]


class DflParticleCapture(C.Structure):
    _fields_ = [("level", C.c_double), ("side", C.c_int32), ("reach", C.c_double), ("T_melt", C.c_double), ("two_way", C.c_int32)]


class DflParticleCaptureStats(C.Structure):
    _fields_ = [("captured", C.c_int64), ("last", C.c_int32)]


class DflSurfaceContact(C.Structure):
    _fields_ = [("level", C.c_double), ("side", C.c_int32), ("T_solid", C.c_double)]


class DflSurfaceContactStats(C.Structure):
    _fields_ = [("last", C.c_int32), ("buried", C.c_int32), ("total", C.c_int64)]


def surface_contact_check(level, side, T_solid):
    """DflSurfaceContactCheck (host only): None when the library accepts the configuration, else the reason"""
    why = C.create_string_buffer(160)
    cfg = DflSurfaceContact(float(level), int(side), float(T_solid))
    return None if lib().DflSurfaceContactCheck(C.byref(cfg), why, 160) == 0 else why.value.decode()


class DflLaser(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("dir", C.c_double * 3), ("scan_vel", C.c_double * 3), ("power", C.c_double),
                ("w", C.c_double), ("h", C.c_double), ("r_cut", C.c_double), ("eta_p", C.c_double), ("eta_s", C.c_double),
                ("substrate_groups", C.c_int32)]


class DflLaserTally(C.Structure):
    _fields_ = [("outside", C.c_double), ("absorbed_particles", C.c_double), ("scattered", C.c_double),
                ("substrate", C.c_double), ("reflected", C.c_double), ("missed", C.c_double)]


class DflLaserSurface(C.Structure):
    _fields_ = [("level", C.c_double), ("side", C.c_int32)]


class DflLaserReflection(C.Structure):
    _fields_ = [("max_bounce", C.c_int32), ("model", C.c_int32), ("eps", C.c_double)]


class DflLaserReflectionTally(C.Structure):
    _fields_ = [("absorbed", C.c_double * 9), ("escaped", C.c_double), ("remaining", C.c_double), ("rays", C.c_int32 * 9)]


class DflFluidCoupling(C.Structure):
    _fields_ = [("rho_f", C.c_double), ("mu_f", C.c_double), ("gravity", C.c_double * 3), ("two_way", C.c_int32)]


PC_JACOBI, PC_DECOMPOSITION, PC_AMGX, PC_ILU0, PC_TWOLEVEL = 0x1, 0x2, 0x3, 0x5, 0x6   # PCType values (include/dedflow.h)
ALLREDUCE_FN = C.CFUNCTYPE(None, vp, vp, C.c_int32)
HALO_FN = C.CFUNCTYPE(None, vp, vp)
STREAM_FN = C.CFUNCTYPE(vp, vp)


class DflAMGXConfig(C.Structure):
    _fields_ = [("relaxation_factor", C.c_double), ("selector_passes", C.c_int32), ("smoother", C.c_int32),
                ("presweeps", C.c_int32), ("postsweeps", C.c_int32), ("max_levels", C.c_int32),
                ("min_coarse_rows", C.c_int32), ("max_iters", C.c_int32), ("unknown_keys", C.c_int32)]


AMGX_SMOOTHER_DILU, AMGX_SMOOTHER_JACOBI = 0, 1


class DflScalarTransport(C.Structure):
    _fields_ = [("phi", C.c_int32), ("T", C.c_int32), ("dirichlet_phi", C.c_int32), ("dirichlet_T", C.c_int32),
                ("pc", C.c_int), ("rtol", C.c_double), ("maxit", C.c_int32)]


class DflSurfaceForces(C.Structure):
    _fields_ = [("level", C.c_double), ("side", C.c_int32), ("eps", C.c_double), ("sigma0", C.c_double),
                ("dsigma_dT", C.c_double), ("T_ref", C.c_double), ("recoil_p0", C.c_double), ("recoil_a", C.c_double),
                ("T_boil", C.c_double), ("h_conv", C.c_double), ("emissivity", C.c_double), ("T_amb", C.c_double),
                ("evap_q0", C.c_double), ("in_time_step", C.c_int32)]


class DflPhaseChange(C.Structure):
    _fields_ = [("T_solidus", C.c_double), ("T_liquidus", C.c_double), ("latent", C.c_double), ("darcy_c", C.c_double),
                ("darcy_b", C.c_double), ("use_phi", C.c_int32), ("level", C.c_double), ("side", C.c_int32), ("eps", C.c_double)]


class DflPhaseChangeStats(C.Structure):
    _fields_ = [("liquid_volume", C.c_double), ("T_max", C.c_double), ("molten", C.c_int64), ("lo", C.c_double * 3),
                ("hi", C.c_double * 3)]


class DflThermalMaterial(C.Structure):
    _fields_ = [("k_gas", C.c_double), ("k_solid", C.c_double), ("k_liquid", C.c_double), ("c_gas", C.c_double),
                ("c_metal", C.c_double), ("T_solidus", C.c_double), ("T_liquidus", C.c_double), ("use_phi", C.c_int32),
                ("level", C.c_double), ("side", C.c_int32), ("eps", C.c_double)]


class DflFluidMaterial(C.Structure):
    _fields_ = [("rho_gas", C.c_double), ("rho_metal", C.c_double), ("mu_gas", C.c_double), ("mu_metal", C.c_double),
                ("gravity", C.c_double * 3), ("beta", C.c_double), ("T_ref", C.c_double), ("use_phi", C.c_int32),
                ("level", C.c_double), ("side", C.c_int32), ("eps", C.c_double)]


class DflRedistance(C.Structure):
    _fields_ = [("level", C.c_double), ("band", C.c_double), ("hold_groups", C.c_int32), ("every", C.c_int32)]


class DflRedistanceStats(C.Structure):
    _fields_ = [("facets", C.c_int64), ("band_nodes", C.c_int64), ("max_change", C.c_double), ("grad_dev_before", C.c_double),
                ("grad_dev_after", C.c_double), ("volume_before", C.c_double), ("volume_after", C.c_double)]


class DflVolumeCorrection(C.Structure):
    _fields_ = [("level", C.c_double), ("side", C.c_int32), ("max_shift", C.c_double), ("tol", C.c_double),
                ("target", C.c_double), ("every", C.c_int32), ("track_capture", C.c_int32)]


class DflVolumeCorrectionStats(C.Structure):
    _fields_ = [("status", C.c_int32), ("passes", C.c_int32), ("band_tets", C.c_int64), ("shift", C.c_double),
                ("target", C.c_double), ("volume_before", C.c_double), ("volume_after", C.c_double),
                ("volume_mesh", C.c_double)]


class DflSolidification(C.Structure):
    _fields_ = [("T_front", C.c_double), ("use_phi", C.c_int32), ("level", C.c_double), ("side", C.c_int32),
                ("in_time_step", C.c_int32)]


class DflSolidificationStats(C.Structure):
    _fields_ = [("time", C.c_double), ("updates", C.c_int64), ("frozen", C.c_int64), ("liquid", C.c_int64),
                ("freeze_events_last", C.c_int64), ("melt_events_last", C.c_int64), ("G_min", C.c_double), ("G_max", C.c_double),
                ("cool_min", C.c_double), ("cool_max", C.c_double), ("R_min", C.c_double), ("R_max", C.c_double),
                ("T_peak_max", C.c_double)]


class DflTrackSections(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("normal", C.c_double * 3), ("up", C.c_double * 3), ("num_station", C.c_int32),
                ("station", C.c_double * 64), ("level", C.c_double), ("side", C.c_int32), ("T_fuse", C.c_double),
                ("every", C.c_int32)]


class DflTrackSection(C.Structure):
    _fields_ = [("area_clad", C.c_double), ("area_fused", C.c_double), ("area_scale", C.c_double), ("height", C.c_double),
                ("depth", C.c_double), ("y_lo_clad", C.c_double), ("y_hi_clad", C.c_double), ("y_lo_fused", C.c_double),
                ("y_hi_fused", C.c_double), ("pairs", C.c_int64), ("dilution", C.c_double)]


class DflPorosity(C.Structure):
    _fields_ = [("level", C.c_double), ("side", C.c_int32), ("open_groups", C.c_int32), ("max_pores", C.c_int32),
                ("every", C.c_int32)]


class DflPore(C.Structure):
    _fields_ = [("label", C.c_int32), ("nodes", C.c_int32), ("tets", C.c_int32), ("volume", C.c_double),
                ("volume_scale", C.c_double), ("lo", C.c_double * 3), ("hi", C.c_double * 3), ("T_wall_min", C.c_double),
                ("T_wall_max", C.c_double)]


class DflPorosityStats(C.Structure):
    _fields_ = [("components", C.c_int64), ("pores", C.c_int64), ("listed", C.c_int64), ("bad_nodes", C.c_int64),
                ("bad_tets", C.c_int64), ("volume_metal", C.c_double), ("volume_open", C.c_double), ("volume_pores", C.c_double),
                ("porosity", C.c_double)]


class dfl_porosity_params(C.Structure):
    _fields_ = [("level", C.c_double), ("side", C.c_double), ("max_pores", C.c_int32)]


class DflSurfaceMesh(C.Structure):
    _fields_ = [("level", C.c_double), ("side", C.c_int32), ("every", C.c_int32)]


class DflSurfaceMeshStats(C.Structure):
    _fields_ = [("vertices", C.c_int64), ("triangles", C.c_int64), ("bad_nodes", C.c_int64), ("bad_tets", C.c_int64),
                ("degenerate_tets", C.c_int64), ("fields", C.c_int64), ("area", C.c_double)]


class dfl_surface_mesh_params(C.Structure):
    _fields_ = [("level", C.c_double), ("side", C.c_double)]


class DflTimeStepLimits(C.Structure):
    _fields_ = [("rate_adv", C.c_double), ("rate_adv_surface", C.c_double), ("cap_q", C.c_double), ("tet_adv", C.c_int32),
                ("tet_surface", C.c_int32), ("tet_cap", C.c_int32), ("num_cut", C.c_int32), ("num_nonfinite", C.c_int32),
                ("dt_adv", C.c_double), ("dt_surface", C.c_double), ("dt_capillary", C.c_double), ("dt", C.c_double)]


class dfl_step_consts(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("dt", "t0", "fact2", "fact2_rho", "fact2_rho2", "fact2_mu4", "fact2_kappa",
                                          "states_old", "corr_old", "corr_new")]


class dfl_step_limit_params(C.Structure):
    _fields_ = [("level", C.c_double), ("sigma0", C.c_double), ("dsigma_dT", C.c_double), ("T_ref", C.c_double)]


class DflComm(C.Structure):
    _fields_ = [("allreduce_sum", ALLREDUCE_FN), ("halo_exchange", HALO_FN), ("ctx", vp), ("num_owned_node", C.c_int32),
                ("halo_begin", HALO_FN), ("halo_end", HALO_FN), ("num_interior_node", C.c_int32),
                ("rank", C.c_int), ("world", C.c_int), ("halo_stream", STREAM_FN)]


def _declare(L):
    def f(name, res, args):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    i32, f64 = C.c_int32, C.c_double
    f("Init", None, [C.c_int, vp]); f("Finalize", None, [])
    f("DflStream", vp, []); f("DflSetStream", None, [vp]); f("DflSetQuiet", None, [i32])
    f("DflSetAssemblySchedule", None, [C.c_int]); f("dfl_set_rhs_lane_grid_cap", None, [C.c_int])
    f("DflMeshSetAssemblySchedule", None, [C.POINTER(Mesh3D), C.c_int]); f("DflMeshSetWeakBCGroup", None, [C.POINTER(Mesh3D), i32])
    f("DflSetWeakBCGroup", None, [i32])
    f("DflSetSlotPatchParameters", None, [i32, i32, i32]); f("DflMeshGeometryChanged", None, [C.POINTER(Mesh3D)])
    f("Mesh3DCreate", C.POINTER(Mesh3D), [i32, i32, i32, i32]); f("Mesh3DDestroy", None, [C.POINTER(Mesh3D)])
    f("Mesh3DUpdateDevice", None, [C.POINTER(Mesh3D)]); f("Mesh3DGenerateColorBatch", None, [C.POINTER(Mesh3D)])
    f("Mesh3DSetBound", None, [C.POINTER(Mesh3D), i32, vp, vp, vp, vp, vp])
    f("CSRAttrCreate", C.POINTER(CSRAttr), [C.POINTER(Mesh3D)]); f("CSRAttrDestroy", None, [C.POINTER(CSRAttr)])
    f("CSRAttrCreateBlock", C.POINTER(CSRAttr), [C.POINTER(CSRAttr), i32, i32])
    f("MatrixCreateTypeCSR", C.POINTER(Matrix), [C.POINTER(CSRAttr), vp])
    f("MatrixCreateTypeFS", C.POINTER(Matrix), [i32, vp, vp])
    f("MatrixDestroy", None, [C.POINTER(Matrix)]); f("MatrixSetup", None, [C.POINTER(Matrix)])
    f("MatrixZero", None, [C.POINTER(Matrix)])
    f("MatrixAMVPBY", None, [C.POINTER(Matrix), f64, vp, f64, vp]); f("MatrixMatVec", None, [C.POINTER(Matrix), vp, vp])
    f("MatrixGetDiag", None, [C.POINTER(Matrix), vp, i32])
    f("MatrixFSBlockValues", vp, [C.POINTER(Matrix)]); f("MatrixFSUseReferenceLayout", None, [C.POINTER(Matrix), i32])
    f("MatrixAddElemValueBlockedBatched", None, [C.POINTER(Matrix), i32, i32, vp, vp, i32, i32, vp, C.c_int, C.c_int, vp])
    f("MatrixMatVecWithMask", None, [C.POINTER(Matrix), vp, vp, vp, vp]); f("MatrixZeroRow", None, [C.POINTER(Matrix), i32, vp, i32, f64])
    f("VecAXPY", None, [f64, vp, vp, i32]); f("VecPointwiseMult", None, [vp, vp, vp, i32]); f("VecPointwiseDiv", None, [vp, vp, vp, i32])
    f("VecPointwiseInv", None, [vp, i32])
    f("MatrixFSExportSubmatrices", None, [C.POINTER(Matrix)]); f("MatrixFSImportSubmatrices", None, [C.POINTER(Matrix)])
    f("DirichletCreate", C.POINTER(Dirichlet), [C.POINTER(Mesh3D), i32, i32]); f("DirichletDestroy", None, [C.POINTER(Dirichlet)])
    f("DirichletApplyVec", None, [C.POINTER(Dirichlet), vp]); f("DirichletApplyMat", None, [C.POINTER(Dirichlet), C.POINTER(Matrix)])
    f("KrylovCreateGMRES", vp, [i32, f64, f64, vp]); f("KrylovCreateCG", vp, [i32, f64, f64, vp])
    f("KrylovDestroy", None, [vp]); f("KrylovSolve", None, [vp, C.POINTER(Matrix), vp, vp])
    f("KrylovGetStats", C.POINTER(KrylovStats), [vp]); f("KrylovSetCheckInterval", None, [vp, i32])
    f("KrylovSetVerbose", None, [vp, i32]); f("KrylovSetComm", None, [vp, C.POINTER(DflComm)])
    f("PCSetup", None, [vp]); f("PCApply", None, [vp, vp, vp]); f("PCDestroy", None, [vp])
    f("PCCreateJacobi", vp, [C.POINTER(Matrix), i32, vp]); f("PCCreateNone", vp, [C.POINTER(Matrix), i32])
    f("PCCreateDILU", vp, [C.POINTER(Matrix)]); f("PCDILUGetColors", i32, [vp, vp]); f("PCDILUGetInverseBlocks", vp, [vp])
    f("KrylovSetPCType", None, [vp, C.c_int]); f("KrylovGetPC", vp, [vp]); f("KrylovSetFusedNorm", None, [vp, C.c_int]); f("KrylovSetPipelined", None, [vp, C.c_int]); f("KrylovSetRestart", None, [vp, i32])
    f("KrylovSetFlexible", None, [vp, i32]); f("KrylovSetMesh", None, [vp, C.POINTER(Mesh3D)]); f("KrylovSetAggregateSize", None, [vp, i32])
    f("PCTwoLevelInfo", None, [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_int64)]); f("PCTwoLevelAggregates", vp, [vp])
    f("PCTwoLevelCoarseMatrix", C.POINTER(Matrix), [vp]); f("PCTwoLevelSetInner", None, [vp, i32, f64])
    f("PCCreateAMGX", vp, [C.POINTER(Matrix), vp]); f("PCAMGXRebuild", None, [vp]); f("PCAMGXNumLevels", i32, [vp])
    f("PCAMGXInfo", None, [vp, vp, vp, vp, C.POINTER(f64), C.POINTER(i32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
    f("PCAMGXLevelAggregates", vp, [vp, i32]); f("PCAMGXLevelColors", vp, [vp, i32])
    f("PCAMGXLevelMatrix", C.POINTER(Matrix), [vp, i32]); f("PCAMGXCoarsePivots", vp, [vp])
    f("DflAMGXParseConfig", C.c_int, [C.c_char_p, C.POINTER(DflAMGXConfig)])
    f("DflAMGXAggregateHost", i32, [i32, vp, vp, vp, C.c_int, vp]); f("KrylovSetAMGXConfig", None, [vp, C.c_char_p])
    f("AssembleSystemTet", None, [C.POINTER(Mesh3D), vp, vp, vp, C.POINTER(Matrix)])
    f("AssembleSystemTetFace", None, [C.POINTER(Mesh3D), vp, vp, vp, C.POINTER(Matrix)])
    f("AssembleSystem", None, [C.POINTER(Mesh3D), vp, vp, vp, C.POINTER(Matrix), vp, i32])
    # kernel-level C ABI used directly by tests / bench
    f("dfl_bcsr_spmv", None, [i32, vp, vp, vp, f64, vp, f64, vp, vp])
    f("dfl_cgs_work_size", C.c_int64, [i32, i32]); f("dfl_reduce_work_size", i32, [])
    f("dfl_cgs_dots", None, [i32, i32, vp, C.c_int64, vp, vp, vp, vp])
    f("dfl_cgs_update", None, [i32, i32, vp, C.c_int64, vp, vp, vp, C.c_int, vp, vp])
    f("dfl_cgs_update_givens", None, [i32, i32, vp, C.c_int64, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp])
    f("dfl_gemv_n", None, [i32, i32, vp, C.c_int64, vp, vp, vp])
    f("dfl_gmres_givens", None, [i32, vp, vp, i32, vp, vp, vp, vp]); f("dfl_gmres_givens_sq", None, [i32, vp, vp, i32, vp, vp, vp, vp])
    f("dfl_gmres_givens_pythagoras", None, [i32, vp, vp, i32, vp, vp, vp, vp, vp])
    f("dfl_cgs_update_pc_givens", None, [i32, i32, i32, vp, C.c_int64, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp])
    f("dfl_cgs_update_pc_givens_x4", None, [i32, i32, i32, vp, C.c_int64, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp])
    f("dfl_gmres_trsv", None, [i32, vp, i32, vp, vp])
    f("dfl_cgs_dots_raw", None, [i32, i32, vp, C.c_int64, vp, vp, vp, vp, vp, vp])
    f("dfl_cgs_update_jacobi_givens", None, [i32, i32, vp, C.c_int64, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp])
    f("dfl_gmres_scale_inv", None, [i32, vp, vp, vp])
    f("dfl_bcsr_spmv_x4", None, [i32, i32, i32, vp, vp, vp, f64, vp, vp, vp])
    f("dfl_bcsr_spmv_x4_scaled", None, [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp])
    f("dfl_interleave4", None, [i32, i32, i32, vp, vp, vp])
    # the products that write M^-1 of their own output (N, rp, ci, diag_pos, val, [d_nrm,] x4, y, z4_out, stream)
    f("dfl_bcsr_spmv_x4_pc", C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp, vp])
    f("dfl_bcsr_spmv_x4_scaled_pc", C.c_int, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp])
    f("dfl_bcsr_diag_pos", None, [i32, vp, vp, vp, vp])
    f("DflKrylovLastFoldedProducts", C.c_int, [vp])
    f("DflKrylovLastFusedBlocks", C.c_int, [vp])
    f("DflKrylovLastGmresStep", C.c_int, [vp])
    f("DflKrylovLastGmresPairs", None, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)])
    f("DflKrylovLastGmresBlocks", None, [vp, C.POINTER(C.c_int * 5), C.POINTER(C.c_int)])
    # blocks of 3 or 4 Arnoldi steps per pass over the raw basis (csrc/k_cgs_block.hip)
    f("dfl_cgs_dots_block_parts", C.c_int, [i32, C.c_int]); f("dfl_cgs_update_block_parts", C.c_int, [i32, C.c_int])
    f("dfl_cgs_dots_block", None, [i32, i32, C.c_int, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp, vp, i32, vp, vp])
    f("dfl_cgs_update_block", None, [i32, i32, C.c_int, vp, C.c_int64, vp, i32, vp, C.c_int64, vp, vp])
    f("dfl_gmres_block_first", None, [C.c_int, vp, C.c_int, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp])
    f("dfl_cgs_fixup_block", None, [i32, C.c_int, vp, C.c_int64, vp, vp, vp, vp, vp, vp])
    f("dfl_gmres_block_second", None, [C.c_int, vp, C.c_int, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp])
    # ... with update and fix-up in one pass (C from the Gram matrix derived in the dots pass)
    f("dfl_cgs_update_fixup_block_parts", C.c_int, [i32])
    f("dfl_cgs_dots_block_gram", None, [i32, i32, C.c_int, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp, vp, i32, vp, vp, vp])
    f("dfl_cgs_update_fixup_block", None, [i32, i32, C.c_int, vp, C.c_int64, vp, i32, vp, C.c_int64, vp, vp, vp, vp, vp, vp])
    f("dfl_gmres_block_fused", None, [C.c_int, vp, C.c_int, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, f64, vp])
    f("dfl_dscal_inv_dev", None, [i32, vp, vp, vp]); f("dfl_dsqrt_dev", None, [vp, vp])
    f("dfl_norms4", None, [i32, vp, vp, C.c_int, vp, vp])
    f("dfl_alpha_states", None, [i32, vp, vp, vp, f64, f64, f64, f64, vp, vp, vp, vp, vp])
    f("dfl_alpha_states2", None, [i32, vp, vp, vp, f64, f64, f64, f64, vp, vp, vp, vp, vp, vp])
    f("dfl_alpha_predict", None, [i32, f64, vp, vp]); f("dfl_alpha_correct", None, [i32, f64, f64, vp, vp, vp, vp])
    f("dfl_ddot", None, [i32, vp, vp, vp, vp, vp]); f("dfl_dnrm2", None, [i32, vp, vp, vp, vp])
    f("dfl_daxpy", None, [i32, f64, vp, vp, vp]); f("dfl_dscal", None, [i32, f64, vp, vp])
    f("dfl_pc_jacobi_setup", None, [i32, vp, vp, vp, vp, vp, vp]); f("dfl_pc_jacobi_apply", None, [i32, i32, vp, vp, vp, vp, vp])
    f("dfl_assemble_tet_lhs", None, [i32, vp, vp, vp, vp, vp, vp])
    f("dfl_assemble_tet_rhs", None, [i32, vp, vp, vp, vp])
    f("dfl_pack_nodes", None, [i32, vp, vp, vp, vp, vp]); f("dfl_unpack_rhs", None, [i32, vp, vp, vp])
    f("ParticleContextCreate", C.POINTER(ParticleContext), [i32]); f("ParticleContextDestroy", None, [C.POINTER(ParticleContext)])
    f("ParticleContextUpdateDevice", None, [C.POINTER(ParticleContext)]); f("ParticleContextUpdateHost", None, [C.POINTER(ParticleContext)])
    f("ParticleContextSetContactModel", None, [C.POINTER(ParticleContext), f64, f64, f64])
    f("ParticleContextComputeForces", None, [C.POINTER(ParticleContext)]); f("ParticleContextUpdate", None, [C.POINTER(ParticleContext)])
    f("ParticleContextSetFluidCoupling", None, [C.POINTER(ParticleContext), C.POINTER(Mesh3D), C.POINTER(DflFluidCoupling)])
    f("ParticleContextLocate", None, [C.POINTER(ParticleContext)]); f("ParticleContextTet", vp, [C.POINTER(ParticleContext)])
    f("ParticleContextBarycentric", vp, [C.POINTER(ParticleContext)]); f("ParticleContextLostCount", i32, [C.POINTER(ParticleContext)])
    f("ParticleContextFluidStep", None, [C.POINTER(ParticleContext), vp]); f("ParticleContextReactionLoad", None, [C.POINTER(ParticleContext), vp])
    f("ParticleContextSetWallMesh", None, [C.POINTER(ParticleContext), C.POINTER(Mesh3D), i32])
    f("ParticleContextWallDroppedCount", i32, [C.POINTER(ParticleContext)])
    f("ParticleContextSetFriction", None, [C.POINTER(ParticleContext), C.POINTER(DflContactFriction)])
    f("ParticleContextAngularVelocity", vp, [C.POINTER(ParticleContext)]); f("ParticleContextAngularAcc", vp, [C.POINTER(ParticleContext)])
    f("ParticleContextFrictionOverflowCount", i32, [C.POINTER(ParticleContext)])
    f("ParticleContextSetGravity", None, [C.POINTER(ParticleContext), C.POINTER(C.c_double)])
    f("ParticleContextSetOutflow", None, [C.POINTER(ParticleContext), C.POINTER(DflParticleOutflow)])
    f("ParticleContextSetInflow", None, [C.POINTER(ParticleContext), C.POINTER(DflParticleInflow)])
    f("ParticleContextAdd", None, [C.POINTER(ParticleContext)]); f("ParticleContextRemove", None, [C.POINTER(ParticleContext)])
    f("ParticleContextFlowStats", None, [C.POINTER(ParticleContext), C.POINTER(DflParticleFlowStats)])
    f("ParticleContextTag", vp, [C.POINTER(ParticleContext)])
    f("ParticleContextSetSizes", None, [C.POINTER(ParticleContext), vp, vp])
    f("ParticleContextRadii", vp, [C.POINTER(ParticleContext)]); f("ParticleContextMasses", vp, [C.POINTER(ParticleContext)])
    f("ParticleContextMaxRadius", f64, [C.POINTER(ParticleContext)])
    f("ParticleContextSetInflowSizes", None, [C.POINTER(ParticleContext), f64, f64])
    f("ParticleContextCopy", None, [C.POINTER(ParticleContext), C.POINTER(ParticleContext)])
    f("ParticleContextFrictionHistory", None, [C.POINTER(ParticleContext), C.POINTER(vp), C.POINTER(C.POINTER(C.c_int32))])
    f("DflMeshSetExternalLoad", None, [C.POINTER(Mesh3D), vp])
    f("ParticleContextSetHeat", None, [C.POINTER(ParticleContext), C.POINTER(DflParticleHeat)])
    f("ParticleContextTemperature", vp, [C.POINTER(ParticleContext)]); f("ParticleContextHeatRate", vp, [C.POINTER(ParticleContext)])
    f("ParticleContextHeatStep", None, [C.POINTER(ParticleContext), vp]); f("ParticleContextHeatSource", None, [C.POINTER(ParticleContext), vp])
    f("DflMeshSetHeatSource", None, [C.POINTER(Mesh3D), vp])
    f("ParticleContextSetLaser", None, [C.POINTER(ParticleContext), C.POINTER(DflLaser)])
    f("ParticleContextLaserStep", None, [C.POINTER(ParticleContext), C.c_double])
    f("ParticleContextLaserRate", vp, [C.POINTER(ParticleContext)])
    f("ParticleContextLaserTally", None, [C.POINTER(ParticleContext), C.POINTER(DflLaserTally)])
    f("ParticleContextLaserColumns", C.c_int32, [C.POINTER(ParticleContext), C.POINTER(vp), C.POINTER(vp)])
    f("ParticleContextSetLaserSurface", None, [C.POINTER(ParticleContext), C.POINTER(DflLaserSurface)])
    f("ParticleContextLaserSurfaceUpdate", C.c_int32, [C.POINTER(ParticleContext), vp])
    f("ParticleContextLaserSurfaceFacets", C.c_int32, [C.POINTER(ParticleContext), C.POINTER(vp), C.POINTER(vp)])
    f("ParticleContextLaserSurfacePower", None, [C.POINTER(ParticleContext), vp])
    f("DflLaserReflectionCheck", C.c_int, [C.POINTER(DflLaserReflection), C.c_char_p, C.c_size_t])
    f("DflLaserReflectionGridStats", None, [C.POINTER(ParticleContext), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                            C.POINTER(C.c_double), C.POINTER(C.c_double)])
    f("ParticleContextSetLaserReflection", None, [C.POINTER(ParticleContext), C.POINTER(DflLaserReflection)])
    f("ParticleContextLaserReflectionTally", None, [C.POINTER(ParticleContext), C.POINTER(DflLaserReflectionTally)])
    f("ParticleContextLaserReflectionRays", C.c_int32, [C.POINTER(ParticleContext), C.POINTER(vp), C.POINTER(vp)])
    f("ParticleContextLaserReflectionFacets", C.c_int32, [C.POINTER(ParticleContext), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)])
    f("ParticleContextSetCapture", None, [C.POINTER(ParticleContext), C.POINTER(DflParticleCapture)])
    f("ParticleContextCapture", i32, [C.POINTER(ParticleContext), vp])
    f("ParticleContextCaptureSource", None, [C.POINTER(ParticleContext), f64, vp, vp, vp])
    f("ParticleContextCaptureStats", None, [C.POINTER(ParticleContext), C.POINTER(DflParticleCaptureStats)])
    f("DflParticleCaptureOn", i32, [C.POINTER(ParticleContext)])
    f("ParticleContextSetSurfaceContact", None, [C.POINTER(ParticleContext), C.POINTER(DflSurfaceContact)])
    f("ParticleContextSurfaceContactStats", None, [C.POINTER(ParticleContext), C.POINTER(DflSurfaceContactStats)])
    f("DflSurfaceContactCheck", C.c_int, [C.POINTER(DflSurfaceContact), C.c_char_p, C.c_size_t])
    f("DflParticleSurfaceContactOn", i32, [C.POINTER(ParticleContext)])
    f("DflSurfaceContactApply", None, [C.POINTER(ParticleContext), vp])
    f("DflSurfaceContactTestNoEarlyExit", None, [C.POINTER(ParticleContext)])
    f("DflMeshSetVolumeSource", None, [C.POINTER(Mesh3D), vp]); f("DflMeshVolumeSource", vp, [C.POINTER(Mesh3D)])
    f("DflParticlePendingEnergy", vp, [C.POINTER(ParticleContext)]); f("DflParticleConductionRate", vp, [C.POINTER(ParticleContext)])
    f("SolveFlowSystem", i32, [C.POINTER(Mesh3D), vp, vp, vp, C.POINTER(Matrix), vp, vp, vp, vp, i32, i32, vp, vp])
    f("DflTimeStep", i32, [C.POINTER(Mesh3D), vp, vp, vp, C.POINTER(Matrix), vp, vp, vp, vp, i32, i32, C.POINTER(ParticleContext),
                           i32, vp, vp])
    f("DflDevicePoolStats", None, [C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
    f("DflKrylovCalibrationLog", C.c_char_p, []); f("DflDeviceMemoryInUse", C.c_int64, []); f("DflWaitDeviceMemoryQuiet", C.c_double, [C.c_double])
    f("DflProfileEnable", None, [C.c_int]); f("DflProfileCollect", C.c_int, [C.c_int, C.POINTER(f64), C.POINTER(f64)])
    f("DflMeshSetScalarTransport", None, [C.POINTER(Mesh3D), C.POINTER(DflScalarTransport)])
    f("DflMeshScalarTransportEnabled", i32, [C.POINTER(Mesh3D)])
    f("DflAssembleScalarJacobian", None, [C.POINTER(Mesh3D), vp, vp, C.POINTER(Matrix), C.POINTER(Matrix)])
    f("DflMeshScalarResidual", vp, [C.POINTER(Mesh3D)])
    f("DflScalarTransportSolve", i32, [C.POINTER(Mesh3D), vp, vp, vp, vp])
    f("DflScalarTransportIterations", None, [C.POINTER(Mesh3D), C.POINTER(i32)])
    f("DflMeshSetSurfaceForces", None, [C.POINTER(Mesh3D), C.POINTER(DflSurfaceForces)])
    f("DflMeshSurfaceForcesEnabled", i32, [C.POINTER(Mesh3D)])
    f("DflMeshSurfaceLoad", None, [C.POINTER(Mesh3D), vp, vp, vp, vp])
    f("DflSurfaceForcesCheck", C.c_int, [C.POINTER(DflSurfaceForces), C.c_char_p, C.c_size_t])
    f("DflMeshSetPhaseChange", None, [C.POINTER(Mesh3D), C.POINTER(DflPhaseChange)])
    f("DflMeshPhaseChangeEnabled", i32, [C.POINTER(Mesh3D)])
    f("DflPhaseChangeCheck", C.c_int, [C.POINTER(DflPhaseChange), C.c_char_p, C.c_size_t])
    f("DflMeshPhaseCoefficients", None, [C.POINTER(Mesh3D), vp, vp, vp, vp])
    f("DflMeshPhaseChangeStats", None, [C.POINTER(Mesh3D), vp, C.POINTER(DflPhaseChangeStats)])
    f("DflMeshSetThermalMaterial", None, [C.POINTER(Mesh3D), C.POINTER(DflThermalMaterial)])
    f("DflMeshThermalMaterialEnabled", i32, [C.POINTER(Mesh3D)])
    f("DflThermalMaterialCheck", C.c_int, [C.POINTER(DflThermalMaterial), C.c_char_p, C.c_size_t])
    f("DflMeshThermalRows", None, [C.POINTER(Mesh3D), vp, vp, vp, vp, vp])
    f("DflMeshSetFluidMaterial", None, [C.POINTER(Mesh3D), C.POINTER(DflFluidMaterial)])
    f("DflMeshFluidMaterialEnabled", i32, [C.POINTER(Mesh3D)])
    f("DflFluidMaterialCheck", C.c_int, [C.POINTER(DflFluidMaterial), C.c_char_p, C.c_size_t])
    f("DflMeshFluidRows", None, [C.POINTER(Mesh3D), vp, vp, vp, vp, vp])
    f("DflMeshSetRedistance", None, [C.POINTER(Mesh3D), C.POINTER(DflRedistance)])
    f("DflMeshRedistanceEnabled", i32, [C.POINTER(Mesh3D)])
    f("DflRedistanceCheck", C.c_int, [C.POINTER(DflRedistance), C.c_char_p, C.c_size_t])
    f("DflMeshRedistance", i32, [C.POINTER(Mesh3D), vp])
    f("DflMeshRedistanceFacets", i32, [C.POINTER(Mesh3D), C.POINTER(vp)])
    f("DflMeshRedistanceStats", None, [C.POINTER(Mesh3D), C.POINTER(DflRedistanceStats)])
    f("DflVolumeCorrectionCheck", C.c_int, [C.POINTER(DflVolumeCorrection), C.c_char_p, C.c_size_t])
    f("DflMeshSetVolumeCorrection", None, [C.POINTER(Mesh3D), C.POINTER(DflVolumeCorrection)])
    f("DflMeshVolumeCorrectionEnabled", i32, [C.POINTER(Mesh3D)])
    f("DflMeshVolumeCorrect", i32, [C.POINTER(Mesh3D), vp])
    f("DflMeshVolumeCorrectionStats", None, [C.POINTER(Mesh3D), C.POINTER(DflVolumeCorrectionStats)])
    f("DflMeshVolumeCorrectionTarget", f64, [C.POINTER(Mesh3D)])
    f("DflMeshVolumeCorrectionSetTarget", None, [C.POINTER(Mesh3D), f64])
    f("DflMeshVolumeCorrectionAddTarget", None, [C.POINTER(Mesh3D), f64])
    f("DflMeshLevelSetVolume", f64, [C.POINTER(Mesh3D), vp, f64])
    f("DflSolidificationCheck", C.c_int, [C.POINTER(DflSolidification), C.c_char_p, C.c_size_t])
    f("DflMeshSetSolidification", None, [C.POINTER(Mesh3D), C.POINTER(DflSolidification)])
    f("DflMeshSolidificationEnabled", i32, [C.POINTER(Mesh3D)])
    f("DflMeshSolidificationUpdate", None, [C.POINTER(Mesh3D), vp, f64])
    f("DflMeshSolidificationReset", None, [C.POINTER(Mesh3D)])
    f("DflMeshSolidificationFields", None, [C.POINTER(Mesh3D)] + 6 * [C.POINTER(vp)])
    f("DflMeshSolidificationEvents", i32, [C.POINTER(Mesh3D), C.POINTER(vp)])
    f("DflMeshSolidificationStats", None, [C.POINTER(Mesh3D), C.POINTER(DflSolidificationStats)])
    f("DflTrackSectionsCheck", C.c_int, [C.POINTER(DflTrackSections), C.c_char_p, C.c_size_t])
    f("DflMeshSetTrackSections", None, [C.POINTER(Mesh3D), C.POINTER(DflTrackSections)])
    f("DflMeshTrackSectionsEnabled", i32, [C.POINTER(Mesh3D)])
    f("DflMeshTrackSectionsStations", i32, [C.POINTER(Mesh3D)])
    f("DflMeshTrackSections", None, [C.POINTER(Mesh3D), vp, vp])
    f("DflMeshTrackSectionsResult", None, [C.POINTER(Mesh3D), C.POINTER(DflTrackSection)])
    f("DflTrackSectionsTestPairs", i32, [C.POINTER(Mesh3D), C.POINTER(vp), C.POINTER(i32)])
    f("DflTrackSectionsTestCapacity", None, [C.POINTER(Mesh3D), C.POINTER(i32), C.POINTER(i32)])
    f("DflPorosityCheck", C.c_int, [C.POINTER(DflPorosity), C.c_char_p, C.c_size_t])
    f("DflMeshSetPorosity", None, [C.POINTER(Mesh3D), C.POINTER(DflPorosity)])
    f("DflMeshPorosityEnabled", i32, [C.POINTER(Mesh3D)])
    f("DflMeshPorosity", i32, [C.POINTER(Mesh3D), vp])
    f("DflMeshPorosityStats", None, [C.POINTER(Mesh3D), C.POINTER(DflPorosityStats)])
    f("DflMeshPorosityResult", i32, [C.POINTER(Mesh3D), C.POINTER(DflPore), i32])
    f("DflMeshPorosityLabels", i32, [C.POINTER(Mesh3D), C.POINTER(vp), C.POINTER(vp)])
    f("DflPorosityTestLaunches", i32, [C.POINTER(Mesh3D)])
    f("DflPorosityTestCapacity", i32, [C.POINTER(Mesh3D), i32])
    pp = C.POINTER(dfl_porosity_params)
    f("dfl_porosity_temp_bytes", C.c_int64, [i32])
    f("dfl_porosity_label", C.c_int, [i32, i32, vp, vp, pp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp])
    f("dfl_porosity_rank", C.c_int, [i32, vp, pp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp])
    f("dfl_porosity_tets", C.c_int, [i32, vp, vp, vp, i32, pp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp])
    f("dfl_porosity_pores", C.c_int, [i32, vp, vp, vp, i32, pp, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, C.c_int64, vp, vp])
    f("DflSurfaceMeshCheck", C.c_int, [C.POINTER(DflSurfaceMesh), C.c_char_p, C.c_size_t])
    f("DflMeshSetSurfaceMesh", None, [C.POINTER(Mesh3D), C.POINTER(DflSurfaceMesh)])
    f("DflMeshSurfaceMeshEnabled", i32, [C.POINTER(Mesh3D)])
    f("DflMeshSurfaceMesh", i32, [C.POINTER(Mesh3D), vp, C.POINTER(vp), i32])
    f("DflMeshSurfaceMeshStats", None, [C.POINTER(Mesh3D), C.POINTER(DflSurfaceMeshStats)])
    f("DflMeshSurfaceMeshArrays", i32, [C.POINTER(Mesh3D)] + 6 * [C.POINTER(vp)] + [C.POINTER(i32)])
    f("DflMeshSurfaceMeshCopy", None, [C.POINTER(Mesh3D), vp, vp, vp])
    f("DflSurfaceMeshTestLaunches", i32, [C.POINTER(Mesh3D)])
    f("DflSurfaceMeshTestGrows", i32, [C.POINTER(Mesh3D), C.POINTER(i32), C.POINTER(i32)])
    f("dfl_surface_mesh_sort_block", i32, [])
    sp = C.POINTER(dfl_surface_mesh_params)
    f("dfl_surface_mesh_temp_bytes", C.c_int64, [i32, i32])
    f("dfl_surface_mesh_count", C.c_int, [i32, i32, vp, vp, vp, sp, vp, vp, vp, vp, vp, vp])
    f("dfl_surface_mesh_build", C.c_int, [i32, i32, vp, vp, vp, sp, vp, vp, i32, i32, vp, vp, i32, vp, C.c_int64, vp, vp, vp,
                                         C.POINTER(vp), i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp])
    f("DflTimeStepCheck", C.c_int, [f64, C.c_char_p, C.c_size_t])
    f("DflMeshSetTimeStep", None, [C.POINTER(Mesh3D), f64]); f("DflMeshTimeStep", f64, [C.POINTER(Mesh3D)])
    f("DflMeshTimeStepLimits", None, [C.POINTER(Mesh3D), vp, f64, C.POINTER(DflTimeStepLimits)])
    f("dfl_step_consts_from_dt", None, [f64, C.POINTER(dfl_step_consts)])
    f("dfl_step_limit_grid", i32, [i32, i32])
    f("dfl_step_limits", None, [i32, vp, vp, vp, i32, C.POINTER(dfl_step_limit_params), i32, vp, vp, vp, vp, vp])
    f("GenerateRandomColor", None, [vp, i32, i32])
    f("dfl_abi_version", C.c_int, [])


def track_sections_config(stations, origin=(0.0, 0.0, 0.0), normal=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), level=0.0, side=1,
                          T_fuse=0.0, every=0, num_station=None):
    """a DflTrackSections; num_station: what the structure claims where that is not len(stations) (the refusals)"""
    st = [float(c) for c in stations]
    cfg = DflTrackSections()
    for k in range(3):
        cfg.origin[k], cfg.normal[k], cfg.up[k] = float(origin[k]), float(normal[k]), float(up[k])
    cfg.num_station = len(st) if num_station is None else int(num_station)
    for k, c in enumerate(st[:64]):
        cfg.station[k] = c
    cfg.level, cfg.side, cfg.T_fuse, cfg.every = float(level), int(side), float(T_fuse), int(every)
    return cfg


def porosity_config(level=0.0, side=1, open_groups=0, max_pores=1024, every=0):
    """a DflPorosity"""
    cfg = DflPorosity()
    cfg.level, cfg.side, cfg.open_groups, cfg.max_pores, cfg.every = float(level), int(side), int(open_groups), int(max_pores), int(every)
    return cfg


def surface_mesh_config(level=0.0, side=1, every=0):
    """a DflSurfaceMesh"""
    cfg = DflSurfaceMesh()
    cfg.level, cfg.side, cfg.every = float(level), int(side), int(every)
    return cfg


BC_STRONG = 1
REFERENCE_BCS = [(0, (1, 1, 1)), (2, (0, 1, 0)), (3, (0, 0, 1)), (4, (0, 0, 0))]  # src/main.c:454-476


class Problem:
    """The reference driver's setup sequence (src/main.c:362-477) through the C API."""

    def __init__(self, mesh, maxit=120, atol=1e-12, rtol=1e-4, quiet=True, bcs=REFERENCE_BCS, color=True, schedule=4,
                 reference_layout=False):
        L = lib()
        L.Init(0, None)
        L.DflSetQuiet(1 if quiet else 0)
        L.DflSetAssemblySchedule(int(schedule))
        self.mesh_np = mesh
        self.N, self.T = mesh.num_node, mesh.num_tet
        self.mesh = L.Mesh3DCreate(self.N, self.T, 0, 0)
        m = self.mesh.contents
        C.memmove(m.host.contents.xg, mesh.xg.ctypes.data, mesh.xg.nbytes)
        C.memmove(m.host.contents.ien, mesh.ien.ctypes.data, mesh.ien.nbytes)
        L.Mesh3DUpdateDevice(self.mesh)
        L.Mesh3DSetBound(self.mesh, mesh.num_bound, mesh.bound_node_offset.ctypes.data, mesh.bound_node.ctypes.data,
                         mesh.bound_elem_offset.ctypes.data, mesh.bound_f2e.ctypes.data, mesh.bound_forn.ctypes.data)
        self.spy1x1 = L.CSRAttrCreate(self.mesh)
        self.spy1x3 = L.CSRAttrCreateBlock(self.spy1x1, 1, 3)
        self.spy3x1 = L.CSRAttrCreateBlock(self.spy1x1, 3, 1)
        self.spy3x3 = L.CSRAttrCreateBlock(self.spy1x1, 3, 3)
        offset = (C.c_int32 * 5)(0, 3, 4, 5, 6)
        self.J = L.MatrixCreateTypeFS(4, offset, None)
        fs = C.cast(self.J.contents.data, C.POINTER(MatrixFS)).contents
        fs.spy1x1 = self.spy1x1
        fs.mat[0] = L.MatrixCreateTypeCSR(self.spy3x3, None)
        fs.mat[1] = L.MatrixCreateTypeCSR(self.spy3x1, None)
        fs.mat[4] = L.MatrixCreateTypeCSR(self.spy1x3, None)
        fs.mat[5] = L.MatrixCreateTypeCSR(self.spy1x1, None)
        if reference_layout:
            L.MatrixFSUseReferenceLayout(self.J, 1)
        L.MatrixSetup(self.J)
        self.fs = fs
        self.nnz1 = int(self.spy1x1.contents.nnz)
        self.ksp = L.KrylovCreateGMRES(maxit, atol, rtol, None)
        L.KrylovSetVerbose(self.ksp, 0 if quiet else 1)
        L.KrylovSetMesh(self.ksp, self.mesh)
        if color:
            L.Mesh3DGenerateColorBatch(self.mesh)
        self.bcs = []
        for group, bctype in bcs:
            bc = L.DirichletCreate(self.mesh, group, 3)
            bt = C.cast(C.addressof(bc.contents) + C.sizeof(Dirichlet), C.POINTER(C.c_int))
            for i, t in enumerate(bctype):
                bt[i] = t
            self.bcs.append(bc)
        self.bc_arr = (C.POINTER(Dirichlet) * len(self.bcs))(*self.bcs)
        sync()

    # ---- integer structure back to numpy -------------------------------------------
    @property
    def num_color(self):
        return int(self.mesh.contents.num_color)

    def color(self):
        return d2h(self.mesh.contents.color, self.T, np.int32)

    def batch_offset(self):
        nc = self.num_color
        return np.ctypeslib.as_array(C.cast(self.mesh.contents.batch_offset, c_i32p), shape=(nc + 1,)).copy()

    def batch_ind(self):
        return d2h(self.mesh.contents.batch_ind, self.T, np.int32)

    def pattern(self, attr=None):
        a = (attr or self.spy1x1).contents
        return d2h(a.row_ptr, a.num_row + 1, np.int32), d2h(a.col_ind, a.nnz, np.int32)

    # ---- values ------------------------------------------------------------------------
    def block_values(self):
        return DeviceArray(self.nnz1 * 16, np.float64, ptr=lib().MatrixFSBlockValues(self.J))

    def export_values(self):
        """The four sub-matrix value arrays in the reference layout (A00, A01, A10, A11)."""
        lib().MatrixFSExportSubmatrices(self.J)   # no-op unless block mode
        sync()
        out = []
        for slot, mult in ((0, 9), (1, 3), (4, 3), (5, 1)):
            csr = C.cast(self.fs.mat[slot].contents.data, C.POINTER(MatrixCSR)).contents
            out.append(d2h(csr.val, self.nnz1 * mult, np.float64))
        return out

    # ---- the hot path --------------------------------------------------------------------
    def assemble_system(self, wg, dwg, F=None, want_J=False):
        lib().AssembleSystem(self.mesh, wg.ptr, dwg.ptr, F.ptr if F is not None else None, self.J if want_J else None,
                             C.cast(self.bc_arr, vp), len(self.bcs))

    def assemble_tet(self, wg, dwg, F=None, want_J=False):
        lib().AssembleSystemTet(self.mesh, wg.ptr, dwg.ptr, F.ptr if F is not None else None, self.J if want_J else None)

    def assemble_face(self, wg, dwg, F=None, want_J=False):
        lib().AssembleSystemTetFace(self.mesh, wg.ptr, dwg.ptr, F.ptr if F is not None else None, self.J if want_J else None)

    def set_external_load(self, load):
        """DflMeshSetExternalLoad: a DeviceArray of 3N (kept alive here while registered), or None"""
        self._ext_load = load
        lib().DflMeshSetExternalLoad(self.mesh, load.ptr if load is not None else None)

    def set_heat_source(self, q):
        """DflMeshSetHeatSource: a DeviceArray of N subtracted from the T rows of every F (kept alive here while registered),
        or None"""
        self._heat_source = q
        lib().DflMeshSetHeatSource(self.mesh, q.ptr if q is not None else None)

    def set_volume_source(self, q):
        """DflMeshSetVolumeSource: a DeviceArray of N (m^3/s per node) subtracted from the p rows of every F (kept alive here
        while registered), or None"""
        self._vol_source = q
        lib().DflMeshSetVolumeSource(self.mesh, q.ptr if q is not None else None)

    def volume_source(self):
        """the registered volume source [N] copied back from the device (None: none registered)"""
        p = lib().DflMeshVolumeSource(self.mesh)
        return d2h(p, self.N, np.float64) if p else None

    def matvec(self, x, y):
        lib().MatrixMatVec(self.J, x.ptr, y.ptr)

    def solve(self, x, b):
        lib().KrylovSolve(self.ksp, self.J, x.ptr, b.ptr)
        st = lib().KrylovGetStats(self.ksp).contents
        it = int(st.iterations)
        return it, float(st.rnrm_init), np.array(st.res_hist[:min(it, 512)]), bool(st.converged)

    def solve_flow_system(self, wgold, dwgold, dwg, F, dx, maxit=4):
        """SolveFlowSystem (src/main.c:77-283); returns (newton_its, rnorm[4], rnorm_init[4])."""
        rn, r0 = (C.c_double * 4)(), (C.c_double * 4)()
        it = lib().SolveFlowSystem(self.mesh, wgold.ptr, dwgold.ptr, dwg.ptr, self.J, F.ptr, dx.ptr, self.ksp,
                                   C.cast(self.bc_arr, vp), len(self.bcs), maxit, C.cast(rn, vp), C.cast(r0, vp))
        return int(it), np.array(rn[:]), np.array(r0[:])

    def time_step(self, wgold, dwgold, dwg, F, dx, newton_maxit=4, particles=None, dem_substeps=0):
        rn, r0 = (C.c_double * 4)(), (C.c_double * 4)()
        it = lib().DflTimeStep(self.mesh, wgold.ptr, dwgold.ptr, dwg.ptr, self.J, F.ptr, dx.ptr, self.ksp, C.cast(self.bc_arr, vp),
                               len(self.bcs), newton_maxit, particles.ctx if particles is not None else None, dem_substeps,
                               C.cast(rn, vp), C.cast(r0, vp))
        return int(it), np.array(rn[:]), np.array(r0[:])

    # ---- time step (include/dedflow.h, "time step") ----------------------------------------------------------------------
    def set_time_step(self, dt):
        """DflMeshSetTimeStep: the step every later call on this problem uses.  A dt the library refuses (not finite, not
        positive; reported on stderr) leaves the step as it was: time_step_size tells."""
        lib().DflMeshSetTimeStep(self.mesh, float(dt))

    def time_step_size(self):
        """DflMeshTimeStep: the step of this problem, DFL_DEFAULT_TIME_STEP until set"""
        return float(lib().DflMeshTimeStep(self.mesh))

    def time_step_limits(self, w, level=0.0):
        """DflMeshTimeStepLimits at the state w (DeviceArray of 6N) and the surface phi = level: a dict of the fields of
        DflTimeStepLimits (synchronises)"""
        s = DflTimeStepLimits()
        lib().DflMeshTimeStepLimits(self.mesh, w.ptr, float(level), C.byref(s))
        return {n: (int if t is C.c_int32 else float)(getattr(s, n)) for n, t in DflTimeStepLimits._fields_}

    # ---- phi / T transport (include/dedflow.h, "scalar transport") -----------------------------------------------------
    def set_scalar_transport(self, phi=True, T=True, dirichlet_phi=(), dirichlet_T=(), pc="jacobi", rtol=1e-10, maxit=200):
        """DflMeshSetScalarTransport: advance phi and / or T in SolveFlowSystem; dirichlet_*: boundary groups whose nodes hold
        their value; pc: "jacobi" or "amgx"."""
        pcs = {"jacobi": PC_JACOBI, "amgx": PC_AMGX}
        if pc not in pcs:
            raise ValueError(f"pc must be one of {sorted(pcs)}")
        cfg = DflScalarTransport(1 if phi else 0, 1 if T else 0, sum(1 << int(g) for g in dirichlet_phi),
                                 sum(1 << int(g) for g in dirichlet_T), pcs[pc], float(rtol), int(maxit))
        lib().DflMeshSetScalarTransport(self.mesh, C.byref(cfg))

    def clear_scalar_transport(self):
        lib().DflMeshSetScalarTransport(self.mesh, None)

    def assemble_scalar_jacobian(self, wg, dwg):
        """DflAssembleScalarJacobian at the alpha states (wg, dwg): the values of Jphi and JT over the nodal pattern
        (self.pattern()), as two numpy arrays."""
        L = lib()
        if getattr(self, "_sj", None) is None:
            self._sj = (L.MatrixCreateTypeCSR(self.spy1x1, None), L.MatrixCreateTypeCSR(self.spy1x1, None))
        L.DflAssembleScalarJacobian(self.mesh, wg.ptr, dwg.ptr, self._sj[0], self._sj[1])
        sync()
        out = []
        for m in self._sj:
            csr = C.cast(m.contents.data, C.POINTER(MatrixCSR)).contents
            out.append(d2h(csr.val, self.nnz1, np.float64))
        return out[0], out[1]

    def scalar_residual(self):
        """DflMeshScalarResidual: the phi / T rows [2N] of the last F assembly (None without a transport)."""
        p = lib().DflMeshScalarResidual(self.mesh)
        sync()
        return d2h(p, 2 * self.N, np.float64) if p else None

    def solve_scalar(self, wgold, dwgold, dwg):
        """DflScalarTransportSolve: one scalar Newton update of dwg[4N:6N) at the current u; returns
        (norms of the phi / T residual it solved against, GMRES iterations of the two solves)."""
        rn = (C.c_double * 2)()
        rc = lib().DflScalarTransportSolve(self.mesh, wgold.ptr, dwgold.ptr, dwg.ptr, C.cast(rn, vp))
        if rc != 0:
            raise RuntimeError("DflScalarTransportSolve refused (no scalar transport set)")
        its = (C.c_int32 * 2)()
        lib().DflScalarTransportIterations(self.mesh, its)
        return np.array(rn[:]), (int(its[0]), int(its[1]))

    # ---- free-surface forces (include/dedflow.h, "free-surface forces") ----------------------------------------------------
    def set_surface_forces(self, level=0.0, side=1, eps=None, sigma0=0.0, dsigma_dT=0.0, T_ref=0.0, recoil_p0=0.0,
                           recoil_a=0.0, T_boil=0.0, h_conv=0.0, emissivity=0.0, T_amb=0.0, evap_q0=0.0, in_time_step=False):
        """DflMeshSetSurfaceForces: surface tension / Marangoni (sigma0, dsigma_dT, T_ref), recoil (recoil_p0, recoil_a,
        T_boil) and heat loss (h_conv, emissivity, T_amb, evap_q0) of the surface phi = level smeared over the half-width eps,
        metal where side (phi - level) > 0; in_time_step: time_step applies them itself.  eps None turns the feature off.  A
        configuration the library refuses (reported on stderr) leaves the mesh as it was: surface_forces_on tells."""
        if eps is None:
            lib().DflMeshSetSurfaceForces(self.mesh, None)
            return
        cfg = DflSurfaceForces(float(level), int(side), float(eps), float(sigma0), float(dsigma_dT), float(T_ref),
                               float(recoil_p0), float(recoil_a), float(T_boil), float(h_conv), float(emissivity), float(T_amb),
                               float(evap_q0), 1 if in_time_step else 0)
        lib().DflMeshSetSurfaceForces(self.mesh, C.byref(cfg))

    @property
    def surface_forces_on(self):
        return bool(lib().DflMeshSurfaceForcesEnabled(self.mesh))

    def surface_load(self, w, want=("load", "heat", "area")):
        """DflMeshSurfaceLoad at the state w (DeviceArray of 6N): a dict of the wanted outputs as DeviceArrays, load [3N],
        heat [N], area [N]; the others are passed as NULL"""
        bad = set(want) - {"load", "heat", "area"}
        if bad:
            raise ValueError(f"surface_load: unknown outputs {sorted(bad)}")
        if not self.surface_forces_on:
            raise RuntimeError("no free-surface forces are set: call set_surface_forces first")
        out = {k: DeviceArray(n * self.N) for k, n in (("load", 3), ("heat", 1), ("area", 1)) if k in want}
        ptr = [out[k].ptr if k in out else None for k in ("load", "heat", "area")]
        lib().DflMeshSurfaceLoad(self.mesh, w.ptr, ptr[0], ptr[1], ptr[2])
        return out

    # ---- phase change (include/dedflow.h, "phase change") ---------------------------------------------------------------------
    def set_phase_change(self, T_solidus=None, T_liquidus=None, latent=0.0, darcy_c=0.0, darcy_b=1e-3, use_phi=False, level=0.0,
                         side=1, eps=1.0):
        """DflMeshSetPhaseChange: latent heat (latent = rho L, J/m^3) and mushy-zone drag (darcy_c, darcy_b) between T_solidus
        and T_liquidus; use_phi: only in the metal, where side (phi - level) > 0, smeared over eps.  T_solidus None turns the
        feature off.  A configuration the library refuses (reported on stderr) leaves the mesh as it was: phase_change_on
        tells."""
        if T_solidus is None:
            lib().DflMeshSetPhaseChange(self.mesh, None)
            return
        cfg = DflPhaseChange(float(T_solidus), float(T_liquidus), float(latent), float(darcy_c), float(darcy_b),
                             1 if use_phi else 0, float(level), int(side), float(eps))
        lib().DflMeshSetPhaseChange(self.mesh, C.byref(cfg))

    @property
    def phase_change_on(self):
        return bool(lib().DflMeshPhaseChangeEnabled(self.mesh))

    def phase_coefficients(self, w, want=("D", "H", "G")):
        """DflMeshPhaseCoefficients at the state w (DeviceArray of 6N): a dict of the wanted outputs as DeviceArrays of N, the
        drag coefficient D, the latent heat capacity H and the liquid volume G; the others are passed as NULL"""
        bad = set(want) - {"D", "H", "G"}
        if bad:
            raise ValueError(f"phase_coefficients: unknown outputs {sorted(bad)}")
        if not self.phase_change_on:
            raise RuntimeError("no phase change is set: call set_phase_change first")
        out = {k: DeviceArray(self.N) for k in ("D", "H", "G") if k in want}
        ptr = [out[k].ptr if k in out else None for k in ("D", "H", "G")]
        lib().DflMeshPhaseCoefficients(self.mesh, w.ptr, ptr[0], ptr[1], ptr[2])
        return out

    def phase_stats(self, w):
        """DflMeshPhaseChangeStats at the state w: liquid_volume, T_max, molten (count), lo [3], hi [3] (synchronises)"""
        if not self.phase_change_on:
            raise RuntimeError("no phase change is set: call set_phase_change first")
        s = DflPhaseChangeStats()
        lib().DflMeshPhaseChangeStats(self.mesh, w.ptr, C.byref(s))
        return dict(liquid_volume=float(s.liquid_volume), T_max=float(s.T_max), molten=int(s.molten), lo=np.array(s.lo[:]),
                    hi=np.array(s.hi[:]))

    # ---- thermal material (include/dedflow.h, "thermal material") -------------------------------------------------------------
    def set_thermal_material(self, k_gas=None, k_solid=None, k_liquid=None, c_gas=None, c_metal=None, T_solidus=0.0,
                             T_liquidus=0.0, use_phi=False, level=0.0, side=1, eps=1.0):
        """DflMeshSetThermalMaterial: conductivities (k_gas, k_solid, k_liquid; k_liquid None: k_solid) and capacities rho cp
        (c_gas, c_metal; c_gas None: c_metal) of the T rows; k between solid and liquid follows the liquid fraction between
        T_solidus and T_liquidus; use_phi: metal where side (phi - level) > 0, smeared over eps, gas elsewhere.  k_solid None
        turns the feature off.  A configuration the library refuses (reported on stderr) leaves the mesh as it was:
        thermal_material_on tells."""
        if k_solid is None:
            lib().DflMeshSetThermalMaterial(self.mesh, None)
            return
        k_liquid = k_solid if k_liquid is None else k_liquid
        k_gas = k_solid if k_gas is None else k_gas
        c_gas = c_metal if c_gas is None else c_gas
        cfg = DflThermalMaterial(float(k_gas), float(k_solid), float(k_liquid), float(c_gas), float(c_metal), float(T_solidus),
                                 float(T_liquidus), 1 if use_phi else 0, float(level), int(side), float(eps))
        lib().DflMeshSetThermalMaterial(self.mesh, C.byref(cfg))

    @property
    def thermal_material_on(self):
        return bool(lib().DflMeshThermalMaterialEnabled(self.mesh))

    def thermal_rows(self, w, dw, want=("r", "Kn", "Cn")):
        """DflMeshThermalRows at (w, dw) taken as the alpha states (DeviceArrays of 6N): a dict of the wanted outputs as
        DeviceArrays of N, the T-row correction r and the nodal totals Kn, Cn; the others are passed as NULL"""
        bad = set(want) - {"r", "Kn", "Cn"}
        if bad:
            raise ValueError(f"thermal_rows: unknown outputs {sorted(bad)}")
        if not self.thermal_material_on:
            raise RuntimeError("no thermal material is set: call set_thermal_material first")
        out = {k: DeviceArray(self.N) for k in ("r", "Kn", "Cn") if k in want}
        ptr = [out[k].ptr if k in out else None for k in ("r", "Kn", "Cn")]
        lib().DflMeshThermalRows(self.mesh, w.ptr, dw.ptr, ptr[0], ptr[1], ptr[2])
        return out

    # ---- fluid material (include/dedflow.h, "fluid material") -----------------------------------------------------------------
    def set_fluid_material(self, rho_gas=None, rho_metal=None, mu_gas=None, mu_metal=None, gravity=(0.0, 0.0, 0.0), beta=0.0,
                           T_ref=0.0, use_phi=False, level=0.0, side=1, eps=1.0):
        """DflMeshSetFluidMaterial: densities (rho_gas None: rho_metal) and viscosities (mu_gas None: mu_metal) of the (u,p)
        rows, the gravity vector and the thermal expansion beta of the metal about T_ref (Boussinesq: only the weight sees
        it); use_phi: metal where side (phi - level) > 0, smeared over eps, gas elsewhere.  rho_metal None turns the feature
        off.  A configuration the library refuses (reported on stderr) leaves the mesh as it was: fluid_material_on tells."""
        if rho_metal is None:
            lib().DflMeshSetFluidMaterial(self.mesh, None)
            return
        rho_gas = rho_metal if rho_gas is None else rho_gas
        mu_gas = mu_metal if mu_gas is None else mu_gas
        cfg = DflFluidMaterial(float(rho_gas), float(rho_metal), float(mu_gas), float(mu_metal),
                               (C.c_double * 3)(*[float(v) for v in gravity]), float(beta), float(T_ref), 1 if use_phi else 0,
                               float(level), int(side), float(eps))
        lib().DflMeshSetFluidMaterial(self.mesh, C.byref(cfg))

    @property
    def fluid_material_on(self):
        return bool(lib().DflMeshFluidMaterialEnabled(self.mesh))

    def fluid_rows(self, w, dw, want=("r", "Rn", "Mn")):
        """DflMeshFluidRows at (w, dw) taken as the alpha states (DeviceArrays of 6N): a dict of the wanted outputs as
        DeviceArrays, the (u,p)-row correction r [4N] and the nodal totals Rn, Mn [N]; the others are passed as NULL"""
        bad = set(want) - {"r", "Rn", "Mn"}
        if bad:
            raise ValueError(f"fluid_rows: unknown outputs {sorted(bad)}")
        if not self.fluid_material_on:
            raise RuntimeError("no fluid material is set: call set_fluid_material first")
        out = {k: DeviceArray(4 * self.N if k == "r" else self.N) for k in ("r", "Rn", "Mn") if k in want}
        ptr = [out[k].ptr if k in out else None for k in ("r", "Rn", "Mn")]
        lib().DflMeshFluidRows(self.mesh, w.ptr, dw.ptr, ptr[0], ptr[1], ptr[2])
        return out

    # ---- level-set redistancing (include/dedflow.h, "level-set redistancing") ----------------------------------------------
    def set_redistance(self, level=None, band=None, hold_groups=0, every=0):
        """DflMeshSetRedistance: the surface phi = level, the half-width band of the rewritten zone, the boundary groups whose
        nodes keep their phi (a bit mask) and, with every > 0, redistancing inside every every-th time_step.  level None turns
        the feature off.  A configuration the library refuses (reported on stderr) leaves the mesh as it was: redistance_on
        tells."""
        if level is None:
            lib().DflMeshSetRedistance(self.mesh, None)
            return
        cfg = DflRedistance(float(level), float(band), int(hold_groups), int(every))
        lib().DflMeshSetRedistance(self.mesh, C.byref(cfg))

    @property
    def redistance_on(self):
        return bool(lib().DflMeshRedistanceEnabled(self.mesh))

    def redistance(self, w):
        """DflMeshRedistance in place on phi of the state w (DeviceArray of 6N, or a raw device pointer); returns the number
        of facets (reads two totals back: synchronises)"""
        if not self.redistance_on:
            raise RuntimeError("no redistancing is set: call set_redistance first")
        return int(lib().DflMeshRedistance(self.mesh, getattr(w, "ptr", w)))

    def redistance_facets(self):
        """the facet list of the last redistance call as a numpy array [nf, 9] (A, B, C of every triangle)"""
        ptr = vp()
        nf = int(lib().DflMeshRedistanceFacets(self.mesh, C.byref(ptr)))
        if nf <= 0:
            return np.zeros((0, 9))
        sync()
        return d2h(ptr.value, 9 * nf, np.float64).reshape(nf, 9)

    def redistance_stats(self):
        """DflMeshRedistanceStats of the last call: facets, band_nodes, max_change, grad_dev_before / _after,
        volume_before / _after (synchronises)"""
        if not self.redistance_on:
            raise RuntimeError("no redistancing is set: call set_redistance first")
        s = DflRedistanceStats()
        lib().DflMeshRedistanceStats(self.mesh, C.byref(s))
        return {k: (int if k in ("facets", "band_nodes") else float)(getattr(s, k)) for k, _ in DflRedistanceStats._fields_}

    def level_set_volume(self, w, level):
        """DflMeshLevelSetVolume: the volume of {phi > level} at the state w (synchronises); needs no configuration"""
        return float(lib().DflMeshLevelSetVolume(self.mesh, getattr(w, "ptr", w), float(level)))

    # ---- level-set volume correction (include/dedflow.h, "level-set volume correction") -----------------------------------
    def set_volume_correction(self, level=None, max_shift=None, tol=1e-10, target=float("nan"), side=1, every=0,
                              track_capture=False):
        """DflMeshSetVolumeCorrection: the surface phi = level, the largest shift a call may apply, the tolerance relative to
        the mesh volume, the volume of {phi > level} to restore (NaN: the first call records it), the metal side and, with
        every > 0, a correction inside every every-th time_step; track_capture lets time_step add what a two-way capture
        deposited to the target.  level None turns the feature off.  A configuration the library refuses (reported on
        stderr) leaves the mesh as it was: volume_correction_on tells."""
        if level is None:
            lib().DflMeshSetVolumeCorrection(self.mesh, None)
            return
        cfg = DflVolumeCorrection(float(level), int(side), float(max_shift), float(tol), float(target), int(every),
                                  int(bool(track_capture)))
        lib().DflMeshSetVolumeCorrection(self.mesh, C.byref(cfg))

    @property
    def volume_correction_on(self):
        return bool(lib().DflMeshVolumeCorrectionEnabled(self.mesh))

    def _need_volume_correction(self):
        if not self.volume_correction_on:
            raise RuntimeError("no volume correction is set: call set_volume_correction first")

    def volume_correct(self, w):
        """DflMeshVolumeCorrect in place on phi of the state w (DeviceArray of 6N, or a raw device pointer); returns the
        status: 0 corrected, 1 already within tolerance, 2 not bracketed, 3 pass limit reached (synchronises)"""
        self._need_volume_correction()
        return int(lib().DflMeshVolumeCorrect(self.mesh, getattr(w, "ptr", w)))

    def volume_correction_stats(self):
        """DflMeshVolumeCorrectionStats of the last call: status (-1: no call yet), passes, band_tets, shift, target,
        volume_before / _after, volume_mesh"""
        self._need_volume_correction()
        s = DflVolumeCorrectionStats()
        lib().DflMeshVolumeCorrectionStats(self.mesh, C.byref(s))
        return {k: (int if k in ("status", "passes", "band_tets") else float)(getattr(s, k))
                for k, _ in DflVolumeCorrectionStats._fields_}

    @property
    def volume_target(self):
        """DflMeshVolumeCorrectionTarget: NaN while it is not recorded"""
        self._need_volume_correction()
        return float(lib().DflMeshVolumeCorrectionTarget(self.mesh))

    @volume_target.setter
    def volume_target(self, volume):
        self._need_volume_correction()
        lib().DflMeshVolumeCorrectionSetTarget(self.mesh, float(volume))

    def add_volume_target(self, dV):
        """DflMeshVolumeCorrectionAddTarget: the target grows by dV of {phi > level}"""
        self._need_volume_correction()
        lib().DflMeshVolumeCorrectionAddTarget(self.mesh, float(dV))

    # ---- solidification record (include/dedflow.h, "solidification record") --------------------------------------------------
    def set_solidification(self, T_front=None, use_phi=False, level=0.0, side=1, in_time_step=False):
        """DflMeshSetSolidification: the per-node record of the last freezing through the isotherm T_front (time, cooling rate,
        recovered thermal gradient), peak temperature, time spent liquid and remelts; use_phi: only in the metal, where
        side (phi - level) > 0; in_time_step: DflTimeStep updates the record itself.  T_front None turns the feature off.  A
        configuration the library refuses (reported on stderr) leaves the mesh as it was: solidification_on tells."""
        if T_front is None:
            lib().DflMeshSetSolidification(self.mesh, None)
            return
        cfg = DflSolidification(float(T_front), 1 if use_phi else 0, float(level), int(side), 1 if in_time_step else 0)
        lib().DflMeshSetSolidification(self.mesh, C.byref(cfg))

    @property
    def solidification_on(self):
        return bool(lib().DflMeshSolidificationEnabled(self.mesh))

    def _need_solidification(self):
        if not self.solidification_on:
            raise RuntimeError("no solidification record is set: call set_solidification first")

    def solidification_update(self, w, dt):
        """DflMeshSolidificationUpdate: w (DeviceArray of 6N, or a device pointer) is the state at the END of a step of
        length dt; the first call after set_solidification or solidification_reset only primes the record"""
        self._need_solidification()
        lib().DflMeshSolidificationUpdate(self.mesh, getattr(w, "ptr", w), float(dt))

    def solidification_reset(self):
        self._need_solidification()
        lib().DflMeshSolidificationReset(self.mesh)

    def solidification_fields(self):
        """numpy copies of the record (synchronises): t_solid, cool, T_peak, t_liquid [N], grad3 [N, 3], melts [N] and the
        derived front speed R = |G| > 0 ? cool / |G| : 0 [N], |G| = sqrt((g0 g0 + g1 g1) + g2 g2)"""
        self._need_solidification()
        p = [vp() for _ in range(6)]
        lib().DflMeshSolidificationFields(self.mesh, *[C.byref(q) for q in p])
        sync()
        N = self.N
        out = {k: d2h(q.value, n * N, t) for k, q, n, t in zip(("t_solid", "grad3", "cool", "T_peak", "t_liquid", "melts"), p,
                                                               (1, 3, 1, 1, 1, 1), 5 * [np.float64] + [np.int32])}
        g = out["grad3"] = out["grad3"].reshape(N, 3)
        G = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            out["R"] = np.where(G > 0.0, out["cool"] / G, 0.0)
        return out

    def solidification_events(self):
        """DflMeshSolidificationEvents: the nodes frozen by the last update, ascending (synchronises)"""
        self._need_solidification()
        p = vp()
        n = int(lib().DflMeshSolidificationEvents(self.mesh, C.byref(p)))
        return d2h(p.value, n, np.int32) if n > 0 else np.zeros(0, np.int32)

    def solidification_stats(self):
        """DflMeshSolidificationStats: time, updates, frozen, liquid, freeze_events_last, melt_events_last, G / cool / R min and
        max over the records, T_peak_max over the metal nodes (synchronises)"""
        self._need_solidification()
        s = DflSolidificationStats()
        lib().DflMeshSolidificationStats(self.mesh, C.byref(s))
        ints = ("updates", "frozen", "liquid", "freeze_events_last", "melt_events_last")
        return {k: (int if k in ints else float)(getattr(s, k)) for k, _ in DflSolidificationStats._fields_}

    # ---- track cross-sections (include/dedflow.h, "track cross-sections") ------------------------------------------------------
    def set_track_sections(self, stations=None, origin=(0.0, 0.0, 0.0), normal=(1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0), level=0.0,
                           side=1, T_fuse=0.0, every=0):
        """DflMeshSetTrackSections: the planes (x - origin) . n = stations[k] (at most 64, strictly ascending) across the scan
        direction `normal`, with `up` the build direction and origin on the original substrate surface; metal where
        side (phi - level) > 0, fused where T_peak >= T_fuse; every > 0: time_step evaluates on every every-th call.  stations
        None turns the feature off.  A configuration the library refuses (reported on stderr) leaves the mesh as it was:
        track_sections_on tells."""
        if stations is None:
            lib().DflMeshSetTrackSections(self.mesh, None)
            return
        lib().DflMeshSetTrackSections(self.mesh, C.byref(track_sections_config(stations, origin, normal, up, level, side, T_fuse,
                                                                             every)))

    @property
    def track_sections_on(self):
        return bool(lib().DflMeshTrackSectionsEnabled(self.mesh))

    def _need_track_sections(self):
        if not self.track_sections_on:
            raise RuntimeError("no track sections are set: call set_track_sections first")

    def track_sections(self, w, T_peak=None):
        """DflMeshTrackSections at the state w (DeviceArray of 6N, or a device pointer); T_peak: a DeviceArray of N or a device
        pointer, None: the solidification record's when one is set, else nothing is fused.  Returns track_sections_result()"""
        self._need_track_sections()
        lib().DflMeshTrackSections(self.mesh, getattr(w, "ptr", w), getattr(T_peak, "ptr", T_peak))
        return self.track_sections_result()

    def track_sections_result(self):
        """DflMeshTrackSectionsResult: one dict per station of the last evaluation (synchronises): area_clad, area_fused,
        area_scale, height, depth, y_lo_clad, y_hi_clad, y_lo_fused, y_hi_fused, pairs, dilution"""
        self._need_track_sections()
        out = (DflTrackSection * 64)()
        lib().DflMeshTrackSectionsResult(self.mesh, out)
        return [{k: (int if k == "pairs" else float)(getattr(r, k)) for k, _ in DflTrackSection._fields_}
                for r in out[:int(lib().DflMeshTrackSectionsStations(self.mesh))]]

    # ---- porosity record (include/dedflow.h, "porosity record") ----------------------------------------------------------------
    def set_porosity(self, level=None, side=1, open_groups=0, max_pores=1024, every=0):
        """DflMeshSetPorosity: metal where side (phi - level) > 0; the gas components that hold a node of a boundary face of a
        group in open_groups (bit g: group g) are open, every other one is a pore; at most max_pores rows are kept, lowest
        labels first; every > 0: time_step evaluates on every every-th call.  level None turns the record off.  A configuration
        the library refuses (reported on stderr) leaves the mesh as it was: porosity_on tells."""
        if level is None:
            lib().DflMeshSetPorosity(self.mesh, None)
            return
        lib().DflMeshSetPorosity(self.mesh, C.byref(porosity_config(level, side, open_groups, max_pores, every)))

    @property
    def porosity_on(self):
        return bool(lib().DflMeshPorosityEnabled(self.mesh))

    def _need_porosity(self):
        if not self.porosity_on:
            raise RuntimeError("no porosity record is set: call set_porosity first")

    def porosity(self, w=None):
        """DflMeshPorosity at the state w (DeviceArray of 6N, or a device pointer; None: the last evaluation).  Returns a dict
        (synchronises): the totals of DflPorosityStats, `list` = one dict per listed pore (label, nodes, tets, volume,
        volume_scale, lo, hi, T_wall_min, T_wall_max), `label` and `pore` = the two [N] int32 arrays of DflMeshPorosityLabels"""
        self._need_porosity()
        L = lib()
        if w is not None:
            L.DflMeshPorosity(self.mesh, getattr(w, "ptr", w))
        s = DflPorosityStats()
        L.DflMeshPorosityStats(self.mesh, C.byref(s))
        out = {k: (float if k.startswith("volume") or k == "porosity" else int)(getattr(s, k)) for k, _ in DflPorosityStats._fields_}
        rows = (DflPore * max(out["listed"], 1))()
        n = int(L.DflMeshPorosityResult(self.mesh, rows, out["listed"]))
        out["list"] = [dict(label=int(r.label), nodes=int(r.nodes), tets=int(r.tets), volume=float(r.volume),
                            volume_scale=float(r.volume_scale), lo=tuple(r.lo), hi=tuple(r.hi), T_wall_min=float(r.T_wall_min),
                            T_wall_max=float(r.T_wall_max)) for r in rows[:n]]
        lab, por = vp(), vp()
        N = int(L.DflMeshPorosityLabels(self.mesh, C.byref(lab), C.byref(por)))
        out["label"], out["pore"] = d2h(lab.value, N, np.int32), d2h(por.value, N, np.int32)
        return out

    # ---- surface mesh (include/dedflow.h, "surface mesh") ------------------------------------------------------------------------
    def set_surface_mesh(self, level=None, side=1, every=0):
        """DflMeshSetSurfaceMesh: metal where side (phi - level) > 0; every > 0: time_step evaluates on every every-th call with
        the field T.  level None turns the section off.  A configuration the library refuses (reported on stderr) leaves the
        mesh as it was: surface_mesh_on tells."""
        if level is None:
            lib().DflMeshSetSurfaceMesh(self.mesh, None)
            return
        lib().DflMeshSetSurfaceMesh(self.mesh, C.byref(surface_mesh_config(level, side, every)))

    @property
    def surface_mesh_on(self):
        return bool(lib().DflMeshSurfaceMeshEnabled(self.mesh))

    def surface_mesh(self, w=None, fields=()):
        """DflMeshSurfaceMesh at the state w (DeviceArray of 6N, or a device pointer; None: the last evaluation) with the nodal
        fields (DeviceArrays of N, or device pointers; at most 8).  Returns a dict (synchronises): the totals of
        DflSurfaceMeshStats, verts [nv, 3], edge [nv, 2], t [nv], vals [nv, K], tris [nt, 3], tri_tet [nt].  An evaluation
        the library refuses (reported on stderr) returns None."""
        if not self.surface_mesh_on:
            raise RuntimeError("no surface mesh is set: call set_surface_mesh first")
        L = lib()
        if w is not None:
            ptrs = (vp * max(len(fields), 1))(*[getattr(q, "ptr", q) for q in fields])
            if L.DflMeshSurfaceMesh(self.mesh, getattr(w, "ptr", w), ptrs, len(fields)) < 0:
                return None
        s = DflSurfaceMeshStats()
        L.DflMeshSurfaceMeshStats(self.mesh, C.byref(s))
        out = {k: (float if k == "area" else int)(getattr(s, k)) for k, _ in DflSurfaceMeshStats._fields_}
        p = [vp() for _ in range(6)]
        nv = C.c_int32()
        nt = int(L.DflMeshSurfaceMeshArrays(self.mesh, *[C.byref(q) for q in p], C.byref(nv)))
        nv = int(nv.value)
        assert (nv, nt) == (out["vertices"], out["triangles"])
        verts, tris = np.empty((nv, 3)), np.empty((nt, 3), np.int32)
        K = out["fields"]
        vals = np.empty((nv, K))
        L.DflMeshSurfaceMeshCopy(self.mesh, verts.ctypes.data, vals.ctypes.data if K else None, tris.ctypes.data)
        out.update(verts=verts, vals=vals, tris=tris, edge=d2h(p[1].value, 2 * nv, np.int32).reshape(-1, 2),
                   t=d2h(p[2].value, nv, np.float64), tri_tet=d2h(p[5].value, nt, np.int32))
        return out

    def close(self):
        L = lib()
        sync()
        for m in getattr(self, "_sj", None) or ():
            L.MatrixDestroy(m)
        self._sj = None
        for bc in self.bcs:
            L.DirichletDestroy(bc)
        self.bcs = []
        L.KrylovDestroy(self.ksp)
        L.MatrixDestroy(self.J)
        for a in (self.spy1x1, self.spy1x3, self.spy3x1, self.spy3x3):
            L.CSRAttrDestroy(a)
        L.Mesh3DDestroy(self.mesh)
