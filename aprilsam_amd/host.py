"""Host-side Python mirror of the reference's graph / solver API for this path.

Same names and argument meaning as the C API (aprilsam/aprilsam.h:184-301): a `Graph` holds xyt
nodes and xyt / xytpos factors; `cholesky()` = april_graph_cholesky, `cholesky_inc()` =
april_graph_cholesky_inc, `chi2()` = april_graph_chi2.  Everything goes through the C-ABI of a
shared library that exports the reference's symbols — libaprilsam_amd.so (the product) by default.
The wrapper is ABI-generic on purpose: the parity tests load oracle/_ref/libaprilsam_ref.so (the
unmodified reference) through the very same class, so both sides of a comparison are driven by
identical Python code.

This module is plumbing only: no numerics happen in Python.
"""
import ctypes as C
import os
import os

import numpy as np

from . import abi

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# APRILSAM_AMD_LIB: another build of the same library (tools/sanitize_host.sh points it at the ASan / UBSan build of the host sources)
PRODUCT_LIB = os.environ.get("APRILSAM_AMD_LIB") or os.path.join(_PKG_DIR, "lib", "libaprilsam_amd.so")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def _np_d(a):
    return a.ctypes.data_as(_dp)


def _np_i(a):
    return a.ctypes.data_as(_ip)


def _polar_pad(m, z, W):
    """z [2] and W [4] as the C interface lays a polar measurement of m rows out"""
    zz = np.zeros(2); zz[:m] = np.asarray(z, float).ravel()[:m]
    WW = np.zeros(4); WW[:m * m] = np.asarray(W, float).ravel()[:m * m]
    return zz, WW


def polar_candidates(cands):
    """(kind [n], z [n, 2], W [n, 4]) of a list of (kind, z [m], W [m, m]) in the layout of aprilsam_amd_gate_polar / _associate_polar"""
    kind = np.array([c[0] for c in cands], np.int32)
    z = np.zeros((len(cands), 2)); W = np.zeros((len(cands), 4))
    for i, (k, zz, WW) in enumerate(cands):
        z[i], W[i] = _polar_pad(2 if int(k) == abi.POLAR_RANGE_BEARING else 1, zz, WW)
    return kind, z, W


class MarginalsError(RuntimeError):
    """a negative return of aprilsam_amd_marginals / _joint: .code is the return value"""

    def __init__(self, code, msg=None):
        super().__init__(f"marginals failed: {code} {msg or ''}".strip())
        self.code = code


class LMError(RuntimeError):
    """a negative return of aprilsam_amd_optimize_lm: .code is the return value"""

    def __init__(self, code, msg=None):
        super().__init__(f"optimize_lm failed: {code} {msg or ''}".strip())
        self.code = code


class GncError(RuntimeError):
    """a negative return of aprilsam_amd_optimize_gnc: .code is the return value"""

    def __init__(self, code, msg=None):
        super().__init__(f"optimize_gnc failed: {code} {msg or ''}".strip())
        self.code = code


class ChordalError(RuntimeError):
    """a negative return of aprilsam_amd_initialize_chordal: .code is the return value, .report the report's fields (written on -2 only)"""

    def __init__(self, code, msg=None, report=None):
        super().__init__(f"initialize_chordal failed: {code} {msg or ''}".strip())
        self.code = code
        self.report = report


class SolverLib:
    """A loaded shared library exporting the reference API names."""

    def __init__(self, path=None):
        self.path = path or PRODUCT_LIB
        if not os.path.exists(self.path):
            raise FileNotFoundError(
                f"{self.path} not found — build it first: python -c 'import __graft_entry__ as g; g.build()'")
        self.dll = C.CDLL(self.path, mode=os.RTLD_LOCAL if hasattr(os, "RTLD_LOCAL") else 0)
        d = self.dll
        self.is_product = hasattr(d, "aprilsam_amd_version")
        d.april_graph_create.restype = C.POINTER(abi.Graph)
        d.april_graph_destroy.argtypes = [C.POINTER(abi.Graph)]
        d.april_graph_node_xyt_create.restype = C.POINTER(abi.Node)
        d.april_graph_node_xyt_create.argtypes = [_dp, _dp, _dp]
        d.april_graph_factor_xyt_create.restype = C.POINTER(abi.Factor)
        d.april_graph_factor_xyt_create.argtypes = [C.c_int, C.c_int, _dp, _dp, C.POINTER(abi.Matd3x3)]
        d.april_graph_factor_xytpos_create.restype = C.POINTER(abi.Factor)
        d.april_graph_factor_xytpos_create.argtypes = [C.c_int, _dp, _dp, C.POINTER(abi.Matd3x3)]
        d.april_graph_chi2.restype = C.c_double
        d.april_graph_chi2.argtypes = [C.POINTER(abi.Graph)]
        for name in ("april_graph_cholesky", "april_graph_cholesky_inc"):
            getattr(d, name).argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam)]
            getattr(d, name).restype = None
        d.april_graph_cholesky_inc_solver.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), _ip]
        d.april_graph_cholesky_inc_solver.restype = None
        d.april_graph_cholesky_param_init.argtypes = [C.POINTER(abi.CholeskyParam)]
        d.april_graph_cholesky_param_destory.argtypes = [C.POINTER(abi.CholeskyParam)]
        if self.is_product:
            self._add_node = d.aprilsam_amd_graph_add_node
            self._add_factor = d.aprilsam_amd_graph_add_factor
            d.aprilsam_amd_version.restype = C.c_char_p
            d.aprilsam_amd_get_stats.argtypes = [C.POINTER(abi.CholeskyParam), C.POINTER(abi.Stats)]
            d.aprilsam_amd_set_option.argtypes = [C.c_char_p, C.c_double]
            if hasattr(d, "aprilsam_amd_get_option"):          # (absent from builds of earlier rounds, which tools/ A/B against this one)
                d.aprilsam_amd_get_option.argtypes = [C.c_char_p, _dp]
                d.aprilsam_amd_debug_guard_selftest.argtypes = [C.POINTER(abi.CholeskyParam)]
            d.aprilsam_amd_last_error.argtypes = [C.c_char_p, C.c_int]
            d.aprilsam_amd_batch_resident.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam),
                                                      C.c_int, _dp, _dp]
            for nm in ("begin", "sync", "end"):
                getattr(d, f"aprilsam_amd_resident_{nm}").argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam)]
            d.aprilsam_amd_resident_steps.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, C.c_int]
            d.aprilsam_amd_resident_chi2.argtypes = [C.POINTER(abi.Graph)]
            d.aprilsam_amd_resident_chi2.restype = C.c_double
            d.aprilsam_amd_set_device.argtypes = [C.c_int]
            if hasattr(d, "aprilsam_amd_param_set_device"):
                d.aprilsam_amd_param_set_device.argtypes = [C.POINTER(abi.CholeskyParam), C.c_int]
                d.aprilsam_amd_param_get_device.argtypes = [C.POINTER(abi.CholeskyParam)]
            d.aprilsam_amd_make_lattice.argtypes = [C.POINTER(abi.Graph), C.c_int]
            d.aprilsam_amd_lattice_arrays.argtypes = [C.c_int, _dp, _ip, _ip, _dp, _dp]
            d.aprilsam_amd_graph_from_arrays.argtypes = [C.POINTER(abi.Graph), C.c_int, _dp, C.c_int, _ip, _ip, _dp, _dp]
            if hasattr(d, "aprilsam_amd_graph_node_arrays"):
                d.aprilsam_amd_graph_node_arrays.argtypes = [C.POINTER(abi.Graph), _dp, _dp, _dp]
                d.aprilsam_amd_graph_node_arrays.restype = None
            d.aprilsam_amd_plan_create.restype = C.c_void_p
            d.aprilsam_amd_plan_create.argtypes = [C.c_int, C.c_int, _ip, _dp, C.c_int]
            d.aprilsam_amd_plan_destroy.argtypes = [C.c_void_p]
            d.aprilsam_amd_plan_query.restype = C.c_longlong
            d.aprilsam_amd_plan_query.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.POINTER(C.c_longlong))]
            d.aprilsam_amd_free.argtypes = [C.c_void_p]
            if hasattr(d, "aprilsam_amd_marginals"):          # (defined in the HIP translation unit: absent from the sanitizer build of the host sources)
                d.aprilsam_amd_marginals.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _dp]
                d.aprilsam_amd_marginals_joint.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _ip, _dp]
                d.aprilsam_amd_debug_selinv_runs.argtypes = [C.POINTER(abi.CholeskyParam)]
                d.aprilsam_amd_debug_selinv_runs.restype = C.c_longlong
            if hasattr(d, "aprilsam_amd_marginals_joint_any"):    # (defined in the HIP translation unit)
                d.aprilsam_amd_marginals_joint_any.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _ip, _dp]
                d.aprilsam_amd_gate_xyt.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _ip, _dp, _dp, _dp, _dp]
                d.aprilsam_amd_debug_path_solve_bytes.argtypes = [C.POINTER(abi.CholeskyParam)]
                d.aprilsam_amd_debug_path_solve_bytes.restype = C.c_longlong
            if hasattr(d, "aprilsam_amd_gate_xyt_joint"):         # (defined in the HIP translation unit)
                d.aprilsam_amd_marginals_set.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _dp]
                d.aprilsam_amd_gate_xyt_joint.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _ip, _ip, _dp, _dp, _dp, _dp]
            if hasattr(d, "aprilsam_amd_logdet"):                 # (defined in the HIP translation unit)
                d.aprilsam_amd_logdet.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), _dp]
                d.aprilsam_amd_logdet_sets.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _ip, _dp]
                d.aprilsam_amd_info_gain_xyt.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _ip, _ip, _dp, _dp]
            if hasattr(d, "aprilsam_amd_solve"):                  # (defined in the HIP translation unit)
                d.aprilsam_amd_solve.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, C.c_int, _dp, _dp]
                for nm in ("aprilsam_amd_marginals_cross", "aprilsam_amd_relative_covariances"):
                    getattr(d, nm).argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, C.c_int, _ip, _dp]
                d.aprilsam_amd_factorised_nodes.argtypes = [C.POINTER(abi.CholeskyParam)]
                d.aprilsam_amd_debug_solve_bytes.argtypes = [C.POINTER(abi.CholeskyParam)]
                d.aprilsam_amd_debug_solve_bytes.restype = C.c_longlong
            if hasattr(d, "aprilsam_amd_optimize_lm"):          # (defined in the HIP translation unit)
                d.aprilsam_amd_lm_opts_init.argtypes = [C.POINTER(abi.LmOpts)]
                d.aprilsam_amd_lm_opts_init.restype = None
                d.aprilsam_amd_optimize_lm.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.POINTER(abi.LmOpts),
                                                       C.POINTER(abi.LmReport), _dp]
            if hasattr(d, "aprilsam_amd_optimize_gnc"):         # (defined in the HIP translation unit)
                d.aprilsam_amd_gnc_opts_init.argtypes = [C.POINTER(abi.GncOpts)]
                d.aprilsam_amd_gnc_opts_init.restype = None
                d.aprilsam_amd_optimize_gnc.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.POINTER(abi.GncOpts), C.c_int, _ip,
                                                        C.POINTER(abi.GncReport), _dp, _dp]
                d.aprilsam_amd_debug_graph_captures.argtypes = [C.POINTER(abi.CholeskyParam)]
                d.aprilsam_amd_debug_graph_captures.restype = C.c_longlong
            if hasattr(d, "aprilsam_amd_debug_front_forms"):
                d.aprilsam_amd_debug_front_forms.argtypes = [C.POINTER(abi.CholeskyParam), _ip, C.c_int]
            if hasattr(d, "aprilsam_amd_debug_inc_forms"):
                d.aprilsam_amd_debug_inc_forms.argtypes = [C.POINTER(abi.CholeskyParam), _ip, C.c_int]
            if hasattr(d, "aprilsam_amd_initialize_chordal"):    # (defined in the HIP translation unit)
                d.aprilsam_amd_chordal_opts_init.argtypes = [C.POINTER(abi.ChordalOpts)]
                d.aprilsam_amd_chordal_opts_init.restype = None
                for nm in ("aprilsam_amd_initialize_chordal", "aprilsam_amd_debug_chordal_raw"):
                    getattr(d, nm).argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.POINTER(abi.ChordalOpts),
                                               C.POINTER(abi.ChordalReport), _dp]
            if hasattr(d, "aprilsam_amd_factor_max_create"):
                d.aprilsam_amd_factor_max_create.restype = C.POINTER(abi.Factor)
                d.aprilsam_amd_factor_max_create.argtypes = [C.POINTER(C.POINTER(abi.Factor)), _dp, C.c_int]
            if hasattr(d, "aprilsam_amd_max_selected"):      # (defined in the HIP translation unit)
                d.aprilsam_amd_max_selected.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _ip]
            if hasattr(d, "aprilsam_amd_factor_set_robust"):
                d.aprilsam_amd_factor_set_robust.argtypes = [C.POINTER(abi.Factor), C.c_int, C.c_double]
                d.aprilsam_amd_factor_get_robust.argtypes = [C.POINTER(abi.Factor), C.POINTER(C.c_int), C.POINTER(C.c_double)]
            if hasattr(d, "aprilsam_amd_node_set_fixed"):
                d.aprilsam_amd_node_set_fixed.argtypes = [C.POINTER(abi.Node), C.c_int]
                d.aprilsam_amd_node_get_fixed.argtypes = [C.POINTER(abi.Node)]
            if hasattr(d, "aprilsam_amd_robust_weights"):    # (defined in the HIP translation unit)
                d.aprilsam_amd_robust_weights.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _dp]
            if hasattr(d, "aprilsam_amd_factor_audit"):      # (defined in the HIP translation unit)
                d.aprilsam_amd_factor_audit.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _dp]
            if hasattr(d, "aprilsam_amd_factor_polar_create"):
                d.aprilsam_amd_factor_polar_create.restype = C.POINTER(abi.Factor)
                d.aprilsam_amd_factor_polar_create.argtypes = [C.c_int, C.c_int, C.c_int, _dp, _dp]
                d.aprilsam_amd_factor_get_polar.argtypes = [C.POINTER(abi.Factor), C.POINTER(C.c_int)]
                d.aprilsam_amd_debug_polar_slot.argtypes = [C.c_int, _dp, _dp, _dp, _dp, _dp, _dp]
            if hasattr(d, "aprilsam_amd_factor_gaussian_create"):
                d.aprilsam_amd_factor_gaussian_create.restype = C.POINTER(abi.Factor)
                d.aprilsam_amd_factor_gaussian_create.argtypes = [C.c_int, _ip, _dp, _dp, _dp]
                d.aprilsam_amd_factor_get_gaussian.argtypes = [C.POINTER(abi.Factor), C.POINTER(C.c_int)]
            if hasattr(d, "aprilsam_amd_graph_remove_nodes"):
                d.aprilsam_amd_graph_remove_nodes.argtypes = [C.POINTER(abi.Graph), C.c_int, _ip, _ip]
            if hasattr(d, "aprilsam_amd_marginal_prior"):         # (defined in the HIP translation unit)
                d.aprilsam_amd_marginal_prior.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, C.c_int, C.POINTER(C.c_int), _ip,
                                                          _dp, _dp, _dp]
                d.aprilsam_amd_graph_marginalize.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _ip]
            if hasattr(d, "aprilsam_amd_debug_polar_gate"):
                d.aprilsam_amd_debug_polar_gate.argtypes = [C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
            if hasattr(d, "aprilsam_amd_gate_polar"):             # (defined in the HIP translation unit)
                d.aprilsam_amd_gate_polar.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, _ip, _ip, _ip, _dp, _dp, _dp, _dp]
                d.aprilsam_amd_associate_polar.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.CholeskyParam), C.c_int, C.c_int, _ip, _dp, _dp, C.c_int, _ip,
                                                           C.c_double, C.c_double, _dp, _ip, _dp, _dp]
            d.aprilsam_amd_graph_save_ex.argtypes = [C.POINTER(abi.Graph), C.c_char_p, C.c_ulonglong]
            d.aprilsam_amd_graph_load.restype = C.POINTER(abi.Graph)
            d.aprilsam_amd_graph_load.argtypes = [C.c_char_p]
            d.aprilsam_amd_attr_put_string.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_char_p]
            d.aprilsam_amd_attr_get_string.restype = C.c_char_p
            d.aprilsam_amd_attr_get_string.argtypes = [C.c_void_p, C.c_char_p]
        else:  # the reference + oracle/ref_shim.c helpers
            self._add_node = d.rs_graph_add_node
            self._add_factor = d.rs_graph_add_factor
        d.april_graph_save.argtypes = [C.POINTER(abi.Graph), C.c_char_p]
        d.april_graph_create_from_file.restype = C.POINTER(abi.Graph)
        d.april_graph_create_from_file.argtypes = [C.c_char_p]
        self._add_node.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.Node)]
        self._add_factor.argtypes = [C.POINTER(abi.Graph), C.POINTER(abi.Factor)]
        self._libc = C.CDLL(None)
        self._libc.calloc.restype = C.c_void_p
        self._libc.calloc.argtypes = [C.c_size_t, C.c_size_t]

    # -- product-only helpers -------------------------------------------------------------------
    def version(self):
        return self.dll.aprilsam_amd_version().decode()

    def device_count(self):
        return int(self.dll.aprilsam_amd_device_count())

    def set_option(self, name, value):
        rc = self.dll.aprilsam_amd_set_option(name.encode(), float(value))
        if rc != 0:
            raise ValueError(f"unknown option {name}")

    def get_option(self, name):
        v = C.c_double()
        if self.dll.aprilsam_amd_get_option(name.encode(), C.byref(v)) != 0:
            raise ValueError(f"unknown option {name}")
        return v.value

    def options(self, **kw):
        """context manager: set the given options, restore what they were on the way out"""
        lib = self

        class _Scope:
            def __enter__(self):
                self.saved = {k: lib.get_option(k) for k in kw}
                for k, v in kw.items():
                    lib.set_option(k, v)
                return lib

            def __exit__(self, *exc):
                for k, v in self.saved.items():
                    lib.set_option(k, v)
                return False
        return _Scope()

    def last_error(self):
        """(code, message) of the most recent failed call in this process; (0, "") when there was none"""
        buf = C.create_string_buffer(1024)
        code = int(self.dll.aprilsam_amd_last_error(buf, 1024))
        return code, buf.value.decode()

    def clear_error(self):
        self.dll.aprilsam_amd_clear_error()

    def lattice_arrays(self, K):
        """SURVEY.md §8(d) synthetic Manhattan lattice as arrays (states, fa, fb, z, W)."""
        N = K * K
        F = 2 * K * (K - 1) + 2 * (K - 1) * (K - 1) + 1
        states = np.zeros((N, 3)); fa = np.zeros(F, np.int32); fb = np.zeros(F, np.int32)
        z = np.zeros((F, 3)); W = np.zeros((F, 9))
        n = self.dll.aprilsam_amd_lattice_arrays(K, _np_d(states), _np_i(fa), _np_i(fb), _np_d(z), _np_d(W))
        assert n == F, (n, F)
        return states, fa, fb, z, W

    def new_graph(self):
        return Graph(self)

    def polar_slot(self, kind, pa, pb, z, W):
        """(z_eff [3], W_eff [3, 3]): the xyt slot of a polar factor at poses pa, pb (aprilsam_amd_debug_polar_slot: host only)"""
        ze = np.zeros(3); We = np.zeros(9)
        m = 2 if int(kind) == abi.POLAR_RANGE_BEARING else 1
        zz = np.zeros(2); zz[:m] = np.asarray(z, float).ravel()[:m]
        WW = np.zeros(4); WW[:m * m] = np.asarray(W, float).ravel()[:m * m]
        rc = self.dll.aprilsam_amd_debug_polar_slot(int(kind), _np_d(np.ascontiguousarray(pa, float)), _np_d(np.ascontiguousarray(pb, float)),
                                                    _np_d(zz), _np_d(WW), _np_d(ze), _np_d(We))
        if rc != 0:
            raise ValueError(f"aprilsam_amd_debug_polar_slot failed rc={rc}: {self.last_error()}")
        return ze, We.reshape(3, 3)

    def polar_gate(self, kind, pa, pb, z, W, cov):
        """(ok, d2, S [m, m]): the gate of one polar candidate at poses pa, pb with the 6 x 6 joint block cov (aprilsam_amd_debug_polar_gate:
        host only); ok is False, d2 and S NaN when rho^2 == 0"""
        m = 2 if int(kind) == abi.POLAR_RANGE_BEARING else 1
        zz, WW = _polar_pad(m, z, W)
        d2 = C.c_double(); S = np.zeros(4)
        rc = self.dll.aprilsam_amd_debug_polar_gate(int(kind), _np_d(np.ascontiguousarray(pa, float)), _np_d(np.ascontiguousarray(pb, float)), _np_d(zz), _np_d(WW),
                                                    _np_d(np.ascontiguousarray(cov, float).reshape(36)), C.byref(d2), _np_d(S))
        if rc < 0:
            raise ValueError(f"aprilsam_amd_debug_polar_gate failed rc={rc}: {self.last_error()}")
        return rc == 0, d2.value, S[:m * m].reshape(m, m).copy()

    def load_graph(self, path):
        """april_graph_create_from_file (april_graph.c:398-426); None when the file cannot be read"""
        if not self.is_product:
            self.dll.april_graph_stype_init(); self.dll.stype_register_basic_types()
        p = self.dll.april_graph_create_from_file(os.fsencode(path))
        if not p:
            return None
        g = Graph.__new__(Graph); g.lib = self; g.ptr = p
        return g

    def new_param(self, **kw):
        return Param(self, **kw)


class Param:
    """april_graph_cholesky_param_t, heap allocated as the reference demands (its _destory frees it)."""

    def __init__(self, lib, nthreshold=100, delta_xy=0.1, delta_theta=0.1, show_timing=0):
        self.lib = lib
        mem = lib._libc.calloc(1, C.sizeof(abi.CholeskyParam))
        self.ptr = C.cast(mem, C.POINTER(abi.CholeskyParam))
        lib.dll.april_graph_cholesky_param_init(self.ptr)
        p = self.ptr.contents
        p.nthreshold, p.delta_xy, p.delta_theta, p.show_timing = nthreshold, delta_xy, delta_theta, show_timing

    @property
    def c(self):
        return self.ptr.contents

    def stats(self):
        st = abi.Stats()
        rc = self.lib.dll.aprilsam_amd_get_stats(self.ptr, C.byref(st))
        if rc != 0:
            raise RuntimeError("no solver context for this param yet")
        return st.asdict()

    def graph_captures(self):
        """hipGraphs captured and instantiated for this param so far (aprilsam_amd_debug_graph_captures); -1: no context yet"""
        return int(self.lib.dll.aprilsam_amd_debug_graph_captures(self.ptr))

    def front_forms(self):
        """(fronts [nF, 8], levels): the form every front of this param's batch plan takes in a batch step's launches
        (aprilsam_amd_debug_front_forms; columns as include/aprilsam_amd.h lists them), and per level a dict(n_big, grouped,
        blocks = [(rb, tile of the closing wide update, of the "ahead" update, of the single-block update)])"""
        n = int(self.lib.dll.aprilsam_amd_debug_front_forms(self.ptr, None, 0))
        if n < 0:
            raise RuntimeError("no batch plan for this param")
        buf = np.zeros(n, np.int32)
        assert int(self.lib.dll.aprilsam_amd_debug_front_forms(self.ptr, _np_i(buf), n)) == n
        nF, nL, w, off = (int(v) for v in buf[:4])
        fronts = buf[4:4 + w * nF].reshape(nF, w).copy()
        levels, k = [], off
        for _ in range(nL):
            nob = int(buf[k + 2])
            levels.append(dict(n_big=int(buf[k]), grouped=bool(buf[k + 1]), blocks=[tuple(int(v) for v in buf[k + 3 + 4 * b:k + 7 + 4 * b]) for b in range(nob)]))
            k += 3 + 4 * nob
        return fronts, levels

    INC_PATHS = ("re-plan", "tail+solve", "tail+list", "tail general", "one", "multi", "levels")

    def inc_forms(self):
        """(head, rows): what this param's most recent april_graph_cholesky_inc did (aprilsam_amd_debug_inc_forms; columns as
        include/aprilsam_amd.h lists them).  head: dict(path (one of INC_PATHS), fail, n_factors, a_idx, n_old, n_new, s_idx, threads, one,
        up_multi, dn_multi); rows: one dict per dirty front, in the order the step regenerated them (children first)"""
        n = int(self.lib.dll.aprilsam_amd_debug_inc_forms(self.ptr, None, 0))
        if n < 0:
            raise RuntimeError("no incremental step on this param yet")
        buf = np.zeros(n, np.int32)
        assert int(self.lib.dll.aprilsam_amd_debug_inc_forms(self.ptr, _np_i(buf), n)) == n
        nrow, hw, rw = (int(v) for v in buf[:3])
        names = ("fail", "n_factors", "a_idx", "n_old", "n_new", "s_idx", "threads", "one", "up_multi", "dn_multi")
        head = dict(path=self.INC_PATHS[int(buf[3])], **{k: int(v) for k, v in zip(names, buf[4:hw])})
        cols = ("front", "mode", "nsb", "nub", "old_nub", "mask", "n_own", "n_ch", "inplace", "mid")
        rows = []
        for i in range(nrow):
            r = buf[hw + rw * i:hw + rw * (i + 1)]
            d = {k: int(v) for k, v in zip(cols, r)}
            d["ch_cnu"] = [int(v) for v in r[len(cols):len(cols) + d["n_ch"]]] if d["mode"] else []
            rows.append(d)
        return head, rows

    def destroy(self):
        if self.ptr:
            self.lib.dll.april_graph_cholesky_param_destory(self.ptr)
            self.ptr = None


class Graph:
    def __init__(self, lib):
        self.lib = lib
        self.ptr = lib.dll.april_graph_create()

    # -- construction (aprilsam.h:285-288) --------------------------------------------------------
    def add_node_xyt(self, state, init=None, truth=None):
        s = (C.c_double * 3)(*state)
        i = (C.c_double * 3)(*(init if init is not None else state))
        t = (C.c_double * 3)(*(truth if truth is not None else state))
        n = self.lib.dll.april_graph_node_xyt_create(s, i, t)
        self.lib._add_node(self.ptr, n)
        return self.n_nodes - 1

    @staticmethod
    def _matd(W):
        m = abi.Matd3x3()
        m.nrows = m.ncols = 3
        for k, v in enumerate(np.asarray(W, float).reshape(9)):
            m.data[k] = v
        return m

    def add_factor_xyt(self, a, b, z, W):
        zz = (C.c_double * 3)(*z)
        m = self._matd(W)
        f = self.lib.dll.april_graph_factor_xyt_create(int(a), int(b), zz, None, C.byref(m))
        self.lib._add_factor(self.ptr, f)

    def make_factor_max(self, a, b, zs, Ws, logw):
        """a max-mixture factor on (a, b) (include/aprilsam_amd.h: aprilsam_amd_factor_max_create), NOT added to the graph: one xyt
        component per row of zs [K, 3] / Ws [K, 9], log weights logw [K].  Raises ValueError (message of the library) when refused."""
        zs = np.asarray(zs, float).reshape(-1, 3); Ws = np.asarray(Ws, float).reshape(-1, 9)
        lw = np.ascontiguousarray(logw, float).ravel()
        K = len(zs)
        if len(Ws) != K or len(lw) != K:
            raise ValueError("zs, Ws and logw must have one row per component")
        d = self.lib.dll
        comps = (C.POINTER(abi.Factor) * max(K, 1))()
        for i in range(K):
            zz = (C.c_double * 3)(*zs[i])
            m = self._matd(Ws[i])
            comps[i] = d.april_graph_factor_xyt_create(int(a), int(b), zz, None, C.byref(m))
        f = d.aprilsam_amd_factor_max_create(comps, _np_d(lw), K)
        if not f:
            for i in range(K):          # (a refused call leaves the components with the caller)
                abi.destroy_factor(comps[i])
            code, msg = self.lib.last_error()
            raise ValueError(f"aprilsam_amd_factor_max_create refused its arguments ({code}): {msg}")
        return f

    def add_factor_max(self, a, b, zs, Ws, logw):
        """append a max-mixture factor (make_factor_max); returns its factor index"""
        self.lib._add_factor(self.ptr, self.make_factor_max(a, b, zs, Ws, logw))
        return self.n_factors - 1

    def max_selected(self, param, factors=None):
        """int array: the component each listed factor's most recent linearisation used, -1 for a non-max factor or one not yet
        linearised (include/aprilsam_amd.h: aprilsam_amd_max_selected); all factors when `factors` is None"""
        idx = np.arange(self.n_factors, dtype=np.int32) if factors is None else np.ascontiguousarray(factors, dtype=np.int32).ravel()
        out = np.full(len(idx), -1, np.int32)
        rc = self.lib.dll.aprilsam_amd_max_selected(self.ptr, param.ptr if param is not None else None, len(idx), _np_i(idx), _np_i(out))
        if rc != 0:
            raise RuntimeError(f"aprilsam_amd_max_selected failed rc={rc}: {self.lib.last_error()}")
        return out

    def set_robust(self, i, kind, c=1.0):
        """give factor i a robust loss (include/aprilsam_amd.h: aprilsam_amd_factor_set_robust): kind one of
        abi.ROBUST_* (ROBUST_NONE clears it), c the threshold on sqrt(r'Wr).  Returns the library's code (0, -12, -13)."""
        return int(self.lib.dll.aprilsam_amd_factor_set_robust(self.factor_ptr(i), int(kind), float(c)))

    def get_robust(self, i):
        """(kind, c) of factor i's robust loss; (ROBUST_NONE, 0.0) for a factor without one"""
        k = C.c_int(-1); c = C.c_double(-1)
        self.lib.dll.aprilsam_amd_factor_get_robust(self.factor_ptr(i), C.byref(k), C.byref(c))
        return k.value, c.value

    def robust_weights(self, param, factors=None):
        """float array: the weight each listed factor's most recent linearisation used, -1 for a non-robust factor or one not yet
        linearised (include/aprilsam_amd.h: aprilsam_amd_robust_weights); all factors when `factors` is None"""
        idx = np.arange(self.n_factors, dtype=np.int32) if factors is None else np.ascontiguousarray(factors, dtype=np.int32).ravel()
        out = np.full(len(idx), -1.0)
        rc = self.lib.dll.aprilsam_amd_robust_weights(self.ptr, param.ptr if param is not None else None, len(idx), _np_i(idx), _np_d(out))
        if rc != 0:
            raise RuntimeError(f"aprilsam_amd_robust_weights failed rc={rc}: {self.lib.last_error()}")
        return out

    def factor_audit(self, param, factors=None):
        """(array [n, 4], count): per listed factor chi2, leverage, d2_loo and checkability in the system the last solver call factorised
        (include/aprilsam_amd.h: aprilsam_amd_factor_audit), and how many of the listed factors could not be audited (host-evaluated: a
        row of NaN each).  All factors of the factorised system when `factors` is None: one row per factor of the graph, rows of factors
        added since that call stay NaN.  Raises RuntimeError on a negative code."""
        if factors is None:
            idx = None; out = np.full((self.n_factors, 4), np.nan)
        else:
            idx = np.ascontiguousarray(factors, dtype=np.int32).ravel(); out = np.full((len(idx), 4), np.nan)
        rc = self.lib.dll.aprilsam_amd_factor_audit(self.ptr, param.ptr if param is not None else None, 0 if idx is None else len(idx),
                                                    None if idx is None else _np_i(idx), _np_d(out))
        if rc < 0:
            raise RuntimeError(f"aprilsam_amd_factor_audit failed rc={rc}: {self.lib.last_error()}")
        return out, int(rc)

    def make_factor_polar(self, kind, a, b, z, W):
        """a range / bearing / range-bearing factor, a observing b (include/aprilsam_amd.h: aprilsam_amd_factor_polar_create; DESIGN.md
        section 19), NOT added to the graph: kind one of abi.POLAR_*, z the m measurements, W their m x m information matrix (m = 2 for
        POLAR_RANGE_BEARING, else 1).  Raises ValueError (message of the library) when refused."""
        zz = np.ascontiguousarray(z, float).ravel(); WW = np.ascontiguousarray(W, float).ravel()
        m = 2 if int(kind) == abi.POLAR_RANGE_BEARING else 1
        if int(kind) in (abi.POLAR_RANGE, abi.POLAR_BEARING, abi.POLAR_RANGE_BEARING) and (len(zz) != m or len(WW) != m * m):
            raise ValueError(f"kind {kind} takes {m} measurements and an {m} x {m} W")
        f = self.lib.dll.aprilsam_amd_factor_polar_create(int(kind), int(a), int(b), _np_d(zz), _np_d(WW))
        if not f:
            code, msg = self.lib.last_error()
            raise ValueError(f"aprilsam_amd_factor_polar_create refused its arguments ({code}): {msg}")
        return f

    def add_factor_polar(self, kind, a, b, z, W):
        """append a polar factor (make_factor_polar); returns its factor index"""
        self.lib._add_factor(self.ptr, self.make_factor_polar(kind, a, b, z, W))
        return self.n_factors - 1

    def get_polar(self, i):
        """kind of factor i when it is a polar factor of this library, 0 for any other factor"""
        k = C.c_int(-1)
        self.lib.dll.aprilsam_amd_factor_get_polar(self.factor_ptr(i), C.byref(k))
        return k.value

    def make_factor_gaussian(self, nodes, xbar, eta, Lambda):
        """a dense Gaussian factor on the k listed nodes in information form (include/aprilsam_amd.h: aprilsam_amd_factor_gaussian_create;
        DESIGN.md section 24), NOT added to the graph: xbar [k, 3], eta [3k], Lambda [3k, 3k].  Raises ValueError (message of the library)
        when refused."""
        nn = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
        k = len(nn)
        xb = np.ascontiguousarray(xbar, float).ravel(); et = np.ascontiguousarray(eta, float).ravel(); L = np.ascontiguousarray(Lambda, float).ravel()
        if len(xb) != 3 * k or len(et) != 3 * k or len(L) != 9 * k * k:
            raise ValueError(f"{k} nodes take xbar and eta of {3 * k} entries and a {3 * k} x {3 * k} Lambda")
        f = self.lib.dll.aprilsam_amd_factor_gaussian_create(k, _np_i(nn), _np_d(xb), _np_d(et), _np_d(L))
        if not f:
            code, msg = self.lib.last_error()
            raise ValueError(f"aprilsam_amd_factor_gaussian_create refused its arguments ({code}): {msg}")
        return f

    def add_factor_gaussian(self, nodes, xbar, eta, Lambda):
        """append a dense Gaussian factor (make_factor_gaussian); returns its factor index"""
        self.lib._add_factor(self.ptr, self.make_factor_gaussian(nodes, xbar, eta, Lambda))
        return self.n_factors - 1

    def get_gaussian(self, i):
        """node count of factor i when it is a dense Gaussian factor of this library, 0 for any other factor"""
        k = C.c_int(-1)
        self.lib.dll.aprilsam_amd_factor_get_gaussian(self.factor_ptr(i), C.byref(k))
        return k.value

    def marginal_prior(self, param, remove, cap=None):
        """(keep [nb], xbar [nb, 3], eta [3 nb], Lambda [3 nb, 3 nb]): the dense Gaussian that eliminating the nodes `remove` leaves on their
        Markov blanket, from the linearisation of the param's last factorisation (include/aprilsam_amd.h: aprilsam_amd_marginal_prior).
        cap: room for blanket nodes (abi.MARGINAL_MAX_NODES by default).  Raises RuntimeError on a refusal (the code is its first argument)."""
        rm = np.ascontiguousarray(remove, dtype=np.int32).ravel()
        cap = abi.MARGINAL_MAX_NODES if cap is None else int(cap)
        nk = C.c_int(-1)
        keep = np.full(max(cap, 1), -1, np.int32); xbar = np.full(3 * max(cap, 1), np.nan); eta = np.full(3 * max(cap, 1), np.nan)
        L = np.full(9 * max(cap, 1) ** 2, np.nan)
        rc = self.lib.dll.aprilsam_amd_marginal_prior(self.ptr, param.ptr if param is not None else None, len(rm), _np_i(rm), cap, C.byref(nk), _np_i(keep),
                                                      _np_d(xbar), _np_d(eta), _np_d(L))
        if rc != 0:
            raise RuntimeError(rc, f"aprilsam_amd_marginal_prior failed rc={rc}: {self.lib.last_error()}")
        nb = nk.value
        return keep[:nb].copy(), xbar[:3 * nb].reshape(nb, 3).copy(), eta[:3 * nb].copy(), L[:9 * nb * nb].reshape(3 * nb, 3 * nb).copy()

    def remove_nodes(self, remove):
        """destroy the listed nodes and every factor that names one, close the gaps, renumber (include/aprilsam_amd.h:
        aprilsam_amd_graph_remove_nodes; host only).  Returns new_index [old N]: the new id of every old node, -1 for a removed one.
        Raises ValueError when refused (the graph is untouched then)."""
        rm = np.ascontiguousarray(remove, dtype=np.int32).ravel()
        n_before = self.n_nodes
        idx = np.full(max(n_before, 1), -2, np.int32)
        rc = self.lib.dll.aprilsam_amd_graph_remove_nodes(self.ptr, len(rm), _np_i(rm), _np_i(idx))
        if rc != 0:
            raise ValueError(f"aprilsam_amd_graph_remove_nodes refused its arguments ({rc}): {self.lib.last_error()[1]}")
        return idx[:n_before]

    def marginalize(self, param, remove):
        """take the listed nodes out of the graph and leave their marginal prior on the blanket as a dense Gaussian factor
        (include/aprilsam_amd.h: aprilsam_amd_graph_marginalize).  Returns (factor index or None when the blanket is empty, new_index).
        Raises RuntimeError on a refusal (the code is its first argument; the graph is untouched then)."""
        rm = np.ascontiguousarray(remove, dtype=np.int32).ravel()
        n_before = self.n_nodes
        idx = np.full(max(n_before, 1), -2, np.int32)
        rc = self.lib.dll.aprilsam_amd_graph_marginalize(self.ptr, param.ptr if param is not None else None, len(rm), _np_i(rm), _np_i(idx))
        if rc < 0:
            raise RuntimeError(rc, f"aprilsam_amd_graph_marginalize failed rc={rc}: {self.lib.last_error()}")
        # (0 is "no factor" or index 0: the prior, when there is one, is the graph's last factor)
        has_factor = len(rm) > 0 and self.n_factors > 0 and rc == self.n_factors - 1 and self.get_gaussian(rc) > 0
        return (rc if has_factor else None), idx[:n_before]

    def add_factor_xytpos(self, a, z, W):
        zz = (C.c_double * 3)(*z)
        m = self._matd(W)
        f = self.lib.dll.april_graph_factor_xytpos_create(int(a), zz, None, C.byref(m))
        self.lib._add_factor(self.ptr, f)

    def build_from_arrays(self, states, fa, fb, z, W):
        """Bulk append: N nodes, F factors (fb<0 => xytpos prior on fa)."""
        states = np.ascontiguousarray(states, float); z = np.ascontiguousarray(z, float)
        W = np.ascontiguousarray(W, float).reshape(-1, 9)
        fa = np.ascontiguousarray(fa, np.int32); fb = np.ascontiguousarray(fb, np.int32)
        fn = self.lib.dll.aprilsam_amd_graph_from_arrays if self.lib.is_product else self.lib.dll.rs_build_from_arrays
        fn.argtypes = [C.POINTER(abi.Graph), C.c_int, _dp, C.c_int, _ip, _ip, _dp, _dp]
        fn(self.ptr, len(states), _np_d(states), len(fa), _np_i(fa), _np_i(fb), _np_d(z), _np_d(W))

    def save(self, path, magic_offset=0):
        """april_graph_save (april_graph.c:377-396): True on success"""
        if self.lib.is_product:
            return self.lib.dll.aprilsam_amd_graph_save_ex(self.ptr, os.fsencode(path), int(magic_offset)) == 1
        self.lib.dll.april_graph_stype_init(); self.lib.dll.stype_register_basic_types()
        return self.lib.dll.april_graph_save(self.ptr, os.fsencode(path)) == 1

    def factor_attr_put(self, i, key, value):
        f = self.factor(i)
        slot = C.cast(C.byref(f, abi.Factor.attr.offset), C.POINTER(C.c_void_p))
        rc = self.lib.dll.aprilsam_amd_attr_put_string(slot, key.encode(), value.encode())
        if rc != 0:
            raise RuntimeError(f"attr_put rc={rc}")

    def factor_attr_get(self, i, key):
        v = self.lib.dll.aprilsam_amd_attr_get_string(self.factor(i).attr, key.encode())
        return v.decode() if v is not None else None

    def arrays(self):
        """(states, fa, fb, z, W) of an xyt / xytpos graph, fb = -1 for priors"""
        n, F = self.n_nodes, self.n_factors
        fa = np.zeros(F, np.int32); fb = np.full(F, -1, np.int32); z = np.zeros((F, 3)); W = np.zeros((F, 9))
        for i in range(F):
            f = self.factor(i)
            fa[i] = f.nodes[0]
            if f.nnodes == 2:
                fb[i] = f.nodes[1]
            zz = f.u.z; Wd = f.u.W.contents.data
            for k in range(3):
                z[i, k] = zz[k]
            for k in range(9):
                W[i, k] = Wd[k]
        return self.states(), fa, fb, z, W

    # -- accessors ------------------------------------------------------------------------------
    @property
    def n_nodes(self):
        return self.ptr.contents.nodes.contents.size

    @property
    def n_factors(self):
        return self.ptr.contents.factors.contents.size

    def node(self, i):
        arr = C.cast(self.ptr.contents.nodes.contents.data, C.POINTER(C.POINTER(abi.Node)))
        return arr[i].contents

    def node_ptr(self, i):
        """the node object pointer of node i (what the C entry points that take one node expect)"""
        if not 0 <= int(i) < self.n_nodes:
            raise IndexError(f"node {i} out of range ({self.n_nodes} nodes)")
        arr = C.cast(self.ptr.contents.nodes.contents.data, C.POINTER(C.POINTER(abi.Node)))
        return arr[int(i)]

    def set_fixed(self, i, fixed=True):
        """hold node i constant, or free it again (include/aprilsam_amd.h: aprilsam_amd_node_set_fixed).  Returns
        the library's code (0, -12, -13)."""
        return int(self.lib.dll.aprilsam_amd_node_set_fixed(self.node_ptr(i), int(fixed)))

    def get_fixed(self, i):
        """True when node i is held constant"""
        return bool(self.lib.dll.aprilsam_amd_node_get_fixed(self.node_ptr(i)))

    def factor(self, i):
        arr = C.cast(self.ptr.contents.factors.contents.data, C.POINTER(C.POINTER(abi.Factor)))
        return arr[i].contents

    def factor_ptr(self, i):
        """the factor object pointer of factor i (what the C entry points that take one factor expect)"""
        if not 0 <= int(i) < self.n_factors:
            raise IndexError(f"factor {i} out of range ({self.n_factors} factors)")
        arr = C.cast(self.ptr.contents.factors.contents.data, C.POINTER(C.POINTER(abi.Factor)))
        return arr[int(i)]

    def _gather(self, field):
        n = self.n_nodes
        out = np.empty((n, 3))
        if self.lib.is_product and hasattr(self.lib.dll, "aprilsam_amd_graph_node_arrays"):      # one call instead of n ctypes round trips
            k = ("state", "l_point", "delta_X").index(field)
            args = [None, None, None]; args[k] = _np_d(out)
            self.lib.dll.aprilsam_amd_graph_node_arrays(self.ptr, *args)
            return out
        arr = C.cast(self.ptr.contents.nodes.contents.data, C.POINTER(C.POINTER(abi.Node)))
        for i in range(n):
            p = getattr(arr[i].contents, field)
            out[i, 0], out[i, 1], out[i, 2] = p[0], p[1], p[2]
        return out

    def states(self):
        return self._gather("state")

    def l_points(self):
        return self._gather("l_point")

    def deltas(self):
        return self._gather("delta_X")

    def states_of(self, i):
        st = self.node(i).state
        return [st[0], st[1], st[2]]

    def set_state(self, i, xyt, relinearize=False):
        nd = self.node(i)
        for k in range(3):
            nd.state[k] = xyt[k]
            if relinearize:
                nd.l_point[k] = xyt[k]

    def set_all_states(self, states, relinearize=False):
        for i in range(self.n_nodes):
            self.set_state(i, states[i], relinearize)

    def set_all_W(self, W):
        """edit the information matrices of all xyt / xytpos factors in place (W: [F, 9])"""
        W = np.asarray(W, float).reshape(-1, 9)
        for i in range(self.n_factors):
            Wd = self.factor(i).u.W.contents.data
            for k in range(9):
                Wd[k] = W[i, k]

    # -- solver (aprilsam.h:268-281) -----------------------------------------------------------------
    def chi2(self):
        return float(self.lib.dll.april_graph_chi2(self.ptr))

    def cholesky(self, param):
        self.lib.dll.april_graph_cholesky(self.ptr, param.ptr)

    def cholesky_inc(self, param):
        self.lib.dll.april_graph_cholesky_inc(self.ptr, param.ptr)

    def cholesky_inc_solver(self, param):
        """april_graph_cholesky_inc_solver (aprilsam.c:578-597); neither library reads the idxs argument"""
        self.lib.dll.april_graph_cholesky_inc_solver(self.ptr, param.ptr, None)

    def marginals(self, param, nodes=None):
        """[n, 3, 3] marginal covariances (x, y, theta) of `nodes` (all nodes: None) from the factor of the last solver call on
        `param` (include/aprilsam_amd.h: aprilsam_amd_marginals).  Raises MarginalsError(rc) on a negative return."""
        if nodes is None:
            n = self.n_nodes
            out = np.empty((n, 3, 3))
            rc = self.lib.dll.aprilsam_amd_marginals(self.ptr, param.ptr, 0, None, _np_d(out))
        else:
            idx = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
            out = np.empty((len(idx), 3, 3))
            rc = self.lib.dll.aprilsam_amd_marginals(self.ptr, param.ptr, len(idx), _np_i(idx), _np_d(out))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return out

    def marginals_joint(self, param, a, b):
        """[n, 6, 6] joint covariances of the pairs (a[i], b[i]), a's unknowns first; pairs off the pattern of the factor come back
        NaN (include/aprilsam_amd.h: aprilsam_amd_marginals_joint).  Raises MarginalsError(rc) on a negative return."""
        a = np.ascontiguousarray(a, dtype=np.int32).ravel(); b = np.ascontiguousarray(b, dtype=np.int32).ravel()
        if a.shape != b.shape:
            raise ValueError("a and b must have the same length")
        out = np.empty((len(a), 6, 6))
        rc = self.lib.dll.aprilsam_amd_marginals_joint(self.ptr, param.ptr, len(a), _np_i(a), _np_i(b), _np_d(out))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return out

    def marginals_joint_any(self, param, a, b):
        """[n, 6, 6] joint covariances of the pairs (a[i], b[i]), a's unknowns first, for ANY pairs (a == b allowed), by triangular
        solves along the factor's assembly-tree paths (include/aprilsam_amd.h: aprilsam_amd_marginals_joint_any).  Raises
        MarginalsError(rc) on a negative return."""
        a = np.ascontiguousarray(a, dtype=np.int32).ravel(); b = np.ascontiguousarray(b, dtype=np.int32).ravel()
        if a.shape != b.shape:
            raise ValueError("a and b must have the same length")
        out = np.empty((len(a), 6, 6))
        rc = self.lib.dll.aprilsam_amd_marginals_joint_any(self.ptr, param.ptr, len(a), _np_i(a), _np_i(b), _np_d(out))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return out

    def gate_xyt(self, param, a, b, z, W):
        """Mahalanobis gating of candidate xyt measurements z[i] (3) with information W[i] (3 x 3) between a[i] and b[i]: returns
        d2 [n] = r' S^-1 r and the innovation covariance S [n, 3, 3] (include/aprilsam_amd.h: aprilsam_amd_gate_xyt).  The residual is
        taken at the nodes' states, the covariance at the last solver call's linearisation points.  Raises MarginalsError(rc) on a
        negative return."""
        a = np.ascontiguousarray(a, dtype=np.int32).ravel(); b = np.ascontiguousarray(b, dtype=np.int32).ravel()
        n = len(a)
        z = np.ascontiguousarray(z, dtype=float).reshape(n, 3); W = np.ascontiguousarray(W, dtype=float).reshape(n, 9)
        if b.shape != a.shape:
            raise ValueError("a and b must have the same length")
        d2 = np.empty(n); S = np.empty((n, 3, 3))
        rc = self.lib.dll.aprilsam_amd_gate_xyt(self.ptr, param.ptr, n, _np_i(a), _np_i(b), _np_d(z), _np_d(W), _np_d(d2), _np_d(S))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return d2, S

    def marginals_set(self, param, nodes):
        """[3k, 3k] dense joint covariance of the k listed nodes, node i's unknowns at rows / columns 3i..3i+2 (include/aprilsam_amd.h:
        aprilsam_amd_marginals_set).  Raises MarginalsError(rc) on a negative return."""
        idx = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
        k = len(idx)
        out = np.empty((3 * k, 3 * k))
        rc = self.lib.dll.aprilsam_amd_marginals_set(self.ptr, param.ptr, k, _np_i(idx), _np_d(out))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return out

    def gate_xyt_joint(self, param, hyps):
        """Joint compatibility gating (include/aprilsam_amd.h: aprilsam_amd_gate_xyt_joint).  hyps: a list of hypotheses, each a tuple
        (a [m], b [m], z [m, 3], W [m, 3, 3] or [m, 9]) of candidate xyt measurements.  Returns (bad, [d2_prefix [m] per hypothesis],
        [C [3m, 3m] per hypothesis]); bad counts the hypotheses with a pivot that was not positive.  Raises MarginalsError(rc) on a
        negative return."""
        ms = [len(np.atleast_1d(h[0])) for h in hyps]
        ptr = np.concatenate([[0], np.cumsum(ms)]).astype(np.int32)
        n = int(ptr[-1])
        cat = lambda k, dt, w: np.ascontiguousarray(np.concatenate([np.asarray(h[k], dt).reshape(-1, w) for h in hyps]) if hyps else np.zeros((0, w), dt))
        a, b, z, W = cat(0, np.int32, 1).ravel(), cat(1, np.int32, 1).ravel(), cat(2, float, 3), cat(3, float, 9)
        if not (len(a) == len(b) == len(z) == len(W) == n):
            raise ValueError("a, b, z and W of a hypothesis must have the same length")
        d2 = np.empty(n); Cm = np.empty(int(sum(9 * m * m for m in ms)))
        rc = self.lib.dll.aprilsam_amd_gate_xyt_joint(self.ptr, param.ptr, len(hyps), _np_i(ptr), _np_i(a), _np_i(b), _np_d(z), _np_d(W), _np_d(d2), _np_d(Cm))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        off = np.concatenate([[0], np.cumsum([9 * m * m for m in ms])]).astype(np.int64)
        return rc, [d2[ptr[h]:ptr[h + 1]] for h in range(len(hyps))], [Cm[off[h]:off[h + 1]].reshape(3 * m, 3 * m) for h, m in enumerate(ms)]

    def logdet(self, param):
        """ln det of the factorised system, in nats (include/aprilsam_amd.h: aprilsam_amd_logdet).  Raises MarginalsError(rc) on a negative
        return."""
        out = C.c_double(0.0)
        rc = self.lib.dll.aprilsam_amd_logdet(self.ptr, param.ptr, C.byref(out))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return out.value

    def logdet_sets(self, param, sets):
        """ln det of the joint marginal covariance of every prefix of every node set (include/aprilsam_amd.h: aprilsam_amd_logdet_sets).
        sets: a list of node lists.  Returns (bad, [prefix [k] per set]); bad counts the sets with a pivot that was not positive.  Raises
        MarginalsError(rc) on a negative return."""
        ks = [len(np.atleast_1d(s)) for s in sets]
        ptr = np.concatenate([[0], np.cumsum(ks)]).astype(np.int32)
        nodes = np.ascontiguousarray(np.concatenate([np.asarray(s, np.int32).ravel() for s in sets]) if sets else np.zeros(0, np.int32))
        out = np.empty(int(ptr[-1]))
        rc = self.lib.dll.aprilsam_amd_logdet_sets(self.ptr, param.ptr, len(sets), _np_i(ptr), _np_i(nodes), _np_d(out))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return rc, [out[ptr[h]:ptr[h + 1]] for h in range(len(sets))]

    def info_gain_xyt(self, param, hyps):
        """Expected information gain of adding candidate xyt measurements (include/aprilsam_amd.h: aprilsam_amd_info_gain_xyt).  hyps: a list
        of hypotheses, each a tuple (a [m], b [m], W [m, 3, 3] or [m, 9]); a gate_xyt_joint tuple (a, b, z, W) is taken too, its z unused.
        Returns (bad, [gain_prefix [m] per hypothesis]).  Raises MarginalsError(rc) on a negative return."""
        ms = [len(np.atleast_1d(h[0])) for h in hyps]
        ptr = np.concatenate([[0], np.cumsum(ms)]).astype(np.int32)
        n = int(ptr[-1])
        cat = lambda k, dt, w: np.ascontiguousarray(np.concatenate([np.asarray(h[k], dt).reshape(-1, w) for h in hyps]) if hyps else np.zeros((0, w), dt))
        a, b, W = cat(0, np.int32, 1).ravel(), cat(1, np.int32, 1).ravel(), cat(-1, float, 9)
        if not (len(a) == len(b) == len(W) == n):
            raise ValueError("a, b and W of a hypothesis must have the same length")
        out = np.empty(n)
        rc = self.lib.dll.aprilsam_amd_info_gain_xyt(self.ptr, param.ptr, len(hyps), _np_i(ptr), _np_i(a), _np_i(b), _np_d(W), _np_d(out))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return rc, [out[ptr[h]:ptr[h + 1]] for h in range(len(hyps))]

    def gate_polar(self, param, a, b, kind, z, W):
        """Mahalanobis gating of candidate polar measurements (include/aprilsam_amd.h: aprilsam_amd_gate_polar): kind [n], z [n, 2], W [n, 4]
        (a 1-row kind uses z[i, 0] and W[i, 0]; see polar_candidates).  Returns (unavailable, d2 [n], S [n, 2, 2]).  Raises
        MarginalsError(rc) on a negative return."""
        a = np.ascontiguousarray(a, dtype=np.int32).ravel(); b = np.ascontiguousarray(b, dtype=np.int32).ravel()
        kind = np.ascontiguousarray(kind, dtype=np.int32).ravel()
        n = len(a)
        if b.shape != a.shape or kind.shape != a.shape:
            raise ValueError("a, b and kind must have the same length")
        z = np.ascontiguousarray(z, dtype=float).reshape(n, 2); W = np.ascontiguousarray(W, dtype=float).reshape(n, 4)
        d2 = np.empty(n); S = np.empty((n, 2, 2))
        rc = self.lib.dll.aprilsam_amd_gate_polar(self.ptr, param.ptr, n, _np_i(a), _np_i(b), _np_i(kind), _np_d(z), _np_d(W), _np_d(d2), _np_d(S))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return rc, d2, S

    def associate_polar(self, param, observer, kind, z, W, landmarks, gate1, gate2, matrix=True):
        """Nearest-neighbour association of m polar observations made from `observer` against the nodes `landmarks`
        (include/aprilsam_amd.h: aprilsam_amd_associate_polar).  Returns dict(unavailable, best [m] (index into landmarks or -1), d2_best [m],
        d2_second [m], d2 [m, L] or None).  Raises MarginalsError(rc) on a negative return."""
        kind = np.ascontiguousarray(kind, dtype=np.int32).ravel()
        lm = np.ascontiguousarray(landmarks, dtype=np.int32).ravel()
        m, L = len(kind), len(lm)
        z = np.ascontiguousarray(z, dtype=float).reshape(m, 2); W = np.ascontiguousarray(W, dtype=float).reshape(m, 4)
        d2 = np.empty((m, L)) if matrix else None
        best = np.empty(m, np.int32); d2b = np.empty(m); d2s = np.empty(m)
        rc = self.lib.dll.aprilsam_amd_associate_polar(self.ptr, param.ptr, int(observer), m, _np_i(kind), _np_d(z), _np_d(W), L, _np_i(lm), float(gate1), float(gate2),
                                                       _np_d(d2) if matrix else None, _np_i(best), _np_d(d2b), _np_d(d2s))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return dict(unavailable=rc, best=best, d2_best=d2b, d2_second=d2s, d2=d2)

    SOLVE_MODES = {"full": 0, "forward": 1, "backward": 2}

    def solve(self, param, B, mode="full"):
        """Solve with the factor of the last solver call on `param` (include/aprilsam_amd.h: aprilsam_amd_solve).  B: [3N] or [nrhs, 3N]
        in node order; mode "full" (A^-1 B), "forward" (L^-1, permuted back to node order) or "backward" (L^-T).  Returns an array of
        B's shape.  Raises MarginalsError(rc) on a negative return."""
        B = np.ascontiguousarray(B, dtype=float)
        B2 = B.reshape(1, -1) if B.ndim == 1 else B
        n = self._factorised_nodes(param)
        if B2.ndim != 2 or B2.shape[0] < 1 or (n >= 0 and B2.shape[1] != 3 * n):
            raise ValueError(f"B must have shape [3N] or [nrhs, 3N] with N = {n}, the nodes of the last solver call")
        X = np.empty_like(B2)
        rc = self.lib.dll.aprilsam_amd_solve(self.ptr, param.ptr, self.SOLVE_MODES[mode], B2.shape[0], _np_d(B2), _np_d(X))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return X.reshape(B.shape)

    def _factorised_nodes(self, param):
        """the nodes of the system the retained factor of `param` was made for (what the C entry points call N); -1: no factor"""
        return int(self.lib.dll.aprilsam_amd_factorised_nodes(param.ptr))

    def _anchored(self, fn, param, anchor, nodes):
        if nodes is None:
            out = np.zeros((max(self._factorised_nodes(param), 0), 3, 3))
            rc = fn(self.ptr, param.ptr, int(anchor), 0, None, _np_d(out))
        else:
            idx = np.ascontiguousarray(nodes, dtype=np.int32).ravel()
            out = np.empty((len(idx), 3, 3))
            rc = fn(self.ptr, param.ptr, int(anchor), len(idx), _np_i(idx), _np_d(out))
        if rc < 0:
            raise MarginalsError(rc, self.lib.last_error())
        return out

    def marginals_cross(self, param, anchor, nodes=None):
        """[n, 3, 3] cross-covariances Sigma_{node, anchor} of `nodes` (all nodes: None) with the pose `anchor`, the node's unknowns as
        rows (include/aprilsam_amd.h: aprilsam_amd_marginals_cross).  Raises MarginalsError(rc) on a negative return."""
        return self._anchored(self.lib.dll.aprilsam_amd_marginals_cross, param, anchor, nodes)

    def relative_covariances(self, param, anchor, nodes=None):
        """[n, 3, 3] covariances of the predicted xyt measurement anchor^-1 o node in the anchor's frame, Jacobians at the current states
        (include/aprilsam_amd.h: aprilsam_amd_relative_covariances).  Raises MarginalsError(rc) on a negative return."""
        return self._anchored(self.lib.dll.aprilsam_amd_relative_covariances, param, anchor, nodes)

    def optimize_lm(self, param, trace=False, **opts):
        """Levenberg-Marquardt on the GPU until a stop test holds (include/aprilsam_amd.h: aprilsam_amd_optimize_lm).
        opts: fields of aprilsam_amd_lm_opts_t (max_iters, check_every, lambda0, lambda_max, eta, ftol, xtol), defaults for the rest.
        Returns the report's fields as a dict, plus "trace": an (iterations, 4) array (F at the trial point, rho, lambda used,
        accepted) when trace is true.  Raises LMError(rc) on a negative return."""
        o = abi.LmOpts()
        self.lib.dll.aprilsam_amd_lm_opts_init(C.byref(o))
        for k, v in opts.items():
            if k not in dict(abi.LmOpts._fields_):
                raise TypeError(f"unknown LM option {k}")
            setattr(o, k, v)
        rep = abi.LmReport()
        tr = np.full((max(int(o.max_iters), 1), 4), np.nan) if trace else None
        rc = self.lib.dll.aprilsam_amd_optimize_lm(self.ptr, param.ptr if param is not None else None, C.byref(o), C.byref(rep),
                                                   _np_d(tr) if trace else None)
        if rc < 0:
            raise LMError(rc, self.lib.last_error())
        out = rep.asdict()
        if trace:
            out["trace"] = tr[:rep.iterations].copy()
        return out

    def optimize_gnc(self, param, candidates, trace=False, **opts):
        """Graduated non-convexity on the GPU (include/aprilsam_amd.h: aprilsam_amd_optimize_gnc) with the surrogate
        loss on the graph factors listed in `candidates`.  opts: fields of aprilsam_amd_gnc_opts_t (loss, c, mu_step, max_stages) and of
        its lm member (max_iters per stage, check_every, lambda0, lambda_max, eta, ftol, xtol), defaults for the rest.  Returns the
        report's fields as a dict, plus "weights": w_mu_final(s) per candidate at the returned states, and when trace is true
        "stage_trace": a (stages, 4) array (mu, F on entry, F at the end, LM iterations).  Raises GncError(rc) on a negative return."""
        o = abi.GncOpts()
        self.lib.dll.aprilsam_amd_gnc_opts_init(C.byref(o))
        for k, v in opts.items():
            if k in ("loss", "c", "mu_step", "max_stages"):
                setattr(o, k, v)
            elif k in dict(abi.LmOpts._fields_):
                setattr(o.lm, k, v)
            else:
                raise TypeError(f"unknown GNC option {k}")
        cand = None if candidates is None else np.ascontiguousarray(candidates, dtype=np.int32).ravel()
        n = 0 if cand is None else len(cand)
        rep = abi.GncReport()
        w = np.full(max(n, 1), np.nan)
        tr = np.full((max(int(o.max_stages), 1), 4), np.nan) if trace else None
        rc = self.lib.dll.aprilsam_amd_optimize_gnc(self.ptr, param.ptr if param is not None else None, C.byref(o), n,
                                                    _np_i(cand) if cand is not None else None, C.byref(rep), _np_d(w),
                                                    _np_d(tr) if trace else None)
        if rc < 0:
            raise GncError(rc, self.lib.last_error())
        out = rep.asdict()
        out["weights"] = w[:n].copy()
        if trace:
            out["stage_trace"] = tr[:rep.stages].copy()
        return out

    def initialize_chordal(self, param, rot=False, raw=False, **opts):
        """Chordal initialisation on the GPU (include/aprilsam_amd.h: aprilsam_amd_initialize_chordal).
        opts: fields of aprilsam_amd_chordal_opts_t (stages).  Returns the report's fields as a dict, plus "rot": the (N, 2) array
        (c_i, s_i) of stage 1 when rot is true, or -- through the debug entry point -- "raw": the (2, N, 3) padded solutions of both
        stages when raw is true.  Raises ChordalError(rc) on a negative return."""
        o = abi.ChordalOpts()
        self.lib.dll.aprilsam_amd_chordal_opts_init(C.byref(o))
        for k, v in opts.items():
            if k not in dict(abi.ChordalOpts._fields_):
                raise TypeError(f"unknown chordal option {k}")
            setattr(o, k, v)
        rep = abi.ChordalReport()
        n = self.n_nodes
        pp = param.ptr if param is not None else None
        if raw:
            buf = np.full((2, n, 3), np.nan)
            rc = self.lib.dll.aprilsam_amd_debug_chordal_raw(self.ptr, pp, C.byref(o), C.byref(rep), _np_d(buf))
        else:
            buf = np.full((n, 2), np.nan) if rot else None
            rc = self.lib.dll.aprilsam_amd_initialize_chordal(self.ptr, pp, C.byref(o), C.byref(rep), _np_d(buf) if rot else None)
        if rc < 0:
            raise ChordalError(rc, self.lib.last_error(), rep.asdict() if rc == -2 else None)
        out = rep.asdict()
        if raw:
            out["raw"] = buf
        elif rot:
            out["rot"] = buf
        return out

    def batch_resident(self, param, iters):
        chi2 = np.zeros(iters + 1); ms = np.zeros(iters)
        rc = self.lib.dll.aprilsam_amd_batch_resident(self.ptr, param.ptr, iters, _np_d(chi2), _np_d(ms))
        if rc != 0:
            raise RuntimeError(f"aprilsam_amd_batch_resident failed rc={rc}")
        return chi2, ms

    def destroy(self):
        if self.ptr:
            self.lib.dll.april_graph_destroy(self.ptr)
            self.ptr = None
