"""One-shard device engine: an object wrapper over the C ABI of ``libasb_hip.so``.

``HipEngine`` is the ONLY compute engine of the product.  The host classes
(``posSnapshots`` / ``posComponents``) talk to it through the small method set below, so
the multi-rank host logic can be exercised on CPU by a test double that lives in
``tests/`` (never in this package).
"""
import ctypes
import weakref

import numpy as np

from . import _lib
from ._lib import AsbLibraryError, ptr


class _PinnedBasis(object):
    """Pinned host memory for a streamed basis (asb_host_alloc).  The ndarray views ``HipEngine.components_pinned`` hands out
    keep this object alive through their buffer, so the memory is freed when the engine AND every view have let go of it --
    never under a live view (the context itself never frees a caller-owned buffer: asb_components_stream_into)."""

    def __init__(self, lib, count):
        p = ctypes.c_void_p()
        if lib.asb_host_alloc(int(count), ctypes.byref(p)) != 0 or not p.value:
            raise MemoryError("asb_host_alloc(%d doubles) failed" % count)
        self._lib, self.ptr, self.count = lib, p.value, int(count)
        self._views = []            # weak references to the ctypes arrays the handed-out ndarrays are built on

    def view(self, shape):
        n = int(np.prod(shape))
        assert n <= self.count
        buf = (ctypes.c_double * n).from_address(self.ptr)
        buf._owner = self           # buffer -> owner: the owner lives as long as any ndarray over it
        self._views = [w for w in self._views if w() is not None] + [weakref.ref(buf)]
        return np.frombuffer(buf, dtype=np.float64, count=n).reshape(shape)

    def in_use(self):
        self._views = [w for w in self._views if w() is not None]
        return bool(self._views)

    def __del__(self):
        try:
            if self.ptr:
                self._lib.asb_host_free(ctypes.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


class HipEngine(object):
    """Owns one ``asb_ctx`` = one GPU, one HIP stream, one vertex shard."""

    device_exchange = True      # exchange records live in device memory (torch tensors)

    STREAM_DEFAULT = -1         # ASB_STREAM_DEFAULT: the device's null stream

    def __init__(self, device_id=0, stream=None):
        """stream: None = private stream; an int hipStream_t handle; 0 or STREAM_DEFAULT = the null
        stream (torch's current stream when the caller has not switched streams)."""
        self.lib = _lib.load()
        if self.lib.asb_abi_version() != 1:
            raise AsbLibraryError("libasb_hip.so ABI version mismatch")
        h = ctypes.c_void_p()
        if stream is None:
            sarg = None
        elif stream in (0, self.STREAM_DEFAULT):
            sarg = ctypes.c_void_p(-1)
        else:
            sarg = ctypes.c_void_p(stream)
        rc = self.lib.asb_create(int(device_id), sarg, ctypes.byref(h))
        if rc != 0:
            msg = self.lib.asb_last_error(h).decode() if h else ""
            if h:
                self.lib.asb_destroy(h)
            raise AsbLibraryError("asb_create(device %d) failed with status %d %s -- a gfx950 (MI355X) GPU is "
                                  "required; there is no CPU fallback" % (device_id, rc, msg))
        self.h = h
        self.device_id = int(device_id)
        # the stream the context enqueues on, as torch would name it: None = private, 0 = the null stream, else the handle
        self.stream_handle = None if stream is None else (0 if stream in (0, self.STREAM_DEFAULT) else int(stream))
        self.F = self.n_loc = self.v0 = self.N_glob = self.K = 0

    # ------------------------------------------------------------------ plumbing
    def _ck(self, rc):
        if rc != 0:
            raise RuntimeError("libasb_hip: status %d: %s" % (rc, self.lib.asb_last_error(self.h).decode()))

    @staticmethod
    def _vec(x, shape):
        """``x`` as a contiguous float64 array of that shape.  (``ptr`` is a bare address: the caller keeps the result in a
        local for the length of the C call.)"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == shape
        return x

    def _invm(self, inv_massL):
        return None if inv_massL is None else self._vec(inv_massL, (self.N_glob,))

    @staticmethod
    def _csr(M):
        """(rows, indptr, indices, data) of a scipy CSR matrix as the C ABI reads them."""
        return (int(M.shape[0]), np.ascontiguousarray(M.indptr, dtype=np.int64), np.ascontiguousarray(M.indices, dtype=np.int64),
                np.ascontiguousarray(M.data, dtype=np.float64))

    def close(self):
        if getattr(self, "h", None):
            self.lib.asb_destroy(self.h)      # (synchronises the copy stream; a caller-owned pinned buffer is not freed there)
            self.h = None
        self._pin = None                      # the views that are still alive keep their memory

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        self._ck(self.lib.asb_sync(self.h))

    def prof_reset(self, enable=True):
        self._ck(self.lib.asb_prof_reset(self.h, int(bool(enable))))

    def prof_get(self):
        n, ms = ctypes.c_int64(), ctypes.c_double()
        self._ck(self.lib.asb_prof_get(self.h, ctypes.byref(n), ctypes.byref(ms)))
        return n.value, ms.value

    # ------------------------------------------------------------------ snapshots
    def upload(self, X, v0, n_loc, massL=None):
        X = np.ascontiguousarray(X, dtype=np.float64)
        F, N, three = X.shape
        assert three == 3
        if massL is not None:
            massL = np.ascontiguousarray(massL, dtype=np.float64)
            assert massL.shape == (N,)
        self._ck(self.lib.asb_snapshots_upload(self.h, ptr(X), F, N, int(v0), int(n_loc), ptr(massL)))
        self.F, self.N_glob, self.v0, self.n_loc = F, N, int(v0), int(n_loc)

    def adopt_device(self, dev_ptr, F, n_loc, massL_loc=None, v0=0, N_glob=None):
        """dev_ptr: device address of an (F, n_loc, 3) float64 tensor (reference layout) holding this
        rank's vertices [v0, v0 + n_loc) of N_glob."""
        if massL_loc is not None:
            massL_loc = np.ascontiguousarray(massL_loc, dtype=np.float64)
        N_glob = int(n_loc if N_glob is None else N_glob)
        self._ck(self.lib.asb_snapshots_adopt_dev(self.h, ctypes.c_void_p(dev_ptr), int(F), int(n_loc), ptr(massL_loc),
                                                  int(v0), N_glob))
        self.F, self.N_glob, self.v0, self.n_loc = int(F), N_glob, int(v0), int(n_loc)

    def upload_rest(self, X, v0, n_loc, massL, rest_shape_code, subtract):
        """upload + rest shape in one sweep: (sum(x), sum(x^2) or None)."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        F, N, three = X.shape
        assert three == 3
        if massL is not None:
            massL = np.ascontiguousarray(massL, dtype=np.float64)
            assert massL.shape == (N,)
        sums = np.zeros(2)
        self._ck(self.lib.asb_snapshots_upload_rest(self.h, ptr(X), F, N, int(v0), int(n_loc), ptr(massL), int(rest_shape_code),
                                                    int(bool(subtract)), ptr(sums)))
        self.F, self.N_glob, self.v0, self.n_loc = F, N, int(v0), int(n_loc)
        return float(sums[0]), (float(sums[1]) if sums[1] >= 0 else None)

    def adopt_device_rest(self, dev_ptr, F, n_loc, massL_loc, v0, N_glob, rest_shape_code, subtract):
        if massL_loc is not None:
            massL_loc = np.ascontiguousarray(massL_loc, dtype=np.float64)
        N_glob = int(n_loc if N_glob is None else N_glob)
        sums = np.zeros(2)
        self._ck(self.lib.asb_snapshots_adopt_dev_rest(self.h, ctypes.c_void_p(dev_ptr), int(F), int(n_loc), ptr(massL_loc),
                                                       int(v0), N_glob, int(rest_shape_code), int(bool(subtract)), ptr(sums)))
        self.F, self.N_glob, self.v0, self.n_loc = int(F), N_glob, int(v0), int(n_loc)
        return float(sums[0]), (float(sums[1]) if sums[1] >= 0 else None)

    def center(self, rest_shape_code, subtract):
        s = ctypes.c_double()
        self._ck(self.lib.asb_snapshots_center(self.h, int(rest_shape_code), int(bool(subtract)), ctypes.byref(s)))
        return s.value

    def sqdev(self, mu):
        s = ctypes.c_double()
        self._ck(self.lib.asb_snapshots_sqdev(self.h, float(mu), ctypes.byref(s)))
        return s.value

    def scale(self, a):
        self._ck(self.lib.asb_snapshots_scale(self.h, float(a)))

    def get_mean(self):
        out = np.empty((self.n_loc, 3))
        self._ck(self.lib.asb_snapshots_get_mean(self.h, ptr(out)))
        return out

    def download_snapshots(self):
        out = np.empty((self.F, self.n_loc, 3))
        self._ck(self.lib.asb_snapshots_download(self.h, ptr(out)))
        return out

    # ------------------------------------------------------------------ deflation
    def deflate_begin(self, K, local_support, mode=_lib.DEFLATE_RESIDUAL):
        if getattr(self, "_streaming", False):
            # the streamed basis goes into pinned memory THIS side owns: a buffer some ndarray still looks at is neither
            # freed nor overwritten by the new run -- the run gets a fresh one and the old one dies with its last view
            need = int(K) * int(self.n_loc) * 3
            pin = getattr(self, "_pin", None)
            if need > 0 and (pin is None or pin.count < need or pin.in_use()):
                self._pin = pin = _PinnedBasis(self.lib, need)
            if need > 0:
                self._ck(self.lib.asb_components_stream_into(self.h, ctypes.c_void_p(pin.ptr), pin.count))
        self._ck(self.lib.asb_deflate_begin(self.h, int(K), int(mode), int(bool(local_support))))
        self.K = int(K)
        self.mode = int(mode)

    def xchg_len(self):
        return int(self.lib.asb_deflate_xchg_len(self.h))

    def local_best(self, k, rec_dev_ptr):
        self._ck(self.lib.asb_deflate_local_best(self.h, int(k), ctypes.c_void_p(rec_dev_ptr)))

    def pick(self, k, recs_dev_ptr=None, n_rec=0):
        self._ck(self.lib.asb_deflate_pick(self.h, int(k), ctypes.c_void_p(recs_dev_ptr) if recs_dev_ptr else None,
                                           int(n_rec)))

    def get_pick(self, k):
        i, s = ctypes.c_int64(), ctypes.c_double()
        self._ck(self.lib.asb_deflate_get_pick(self.h, int(k), ctypes.byref(i), ctypes.byref(s)))
        return i.value, s.value

    def block_argmax(self, p):
        """(global block index, energy) of the constraint block with the largest residual energy on this shard."""
        i, v = ctypes.c_int64(), ctypes.c_double()
        self._ck(self.lib.asb_deflate_block_argmax(self.h, int(p), ctypes.byref(i), ctypes.byref(v)))
        return i.value, v.value

    def force_next(self, gidx):
        self._ck(self.lib.asb_deflate_force_next(self.h, int(gidx)))

    def apply(self, k, s_loc=None):
        if s_loc is not None:
            s_loc = np.ascontiguousarray(s_loc, dtype=np.float64)
            assert s_loc.shape == (self.n_loc,)
        self._ck(self.lib.asb_deflate_apply(self.h, int(k), ptr(s_loc)))

    def run_global(self, k0, k1):
        self._ck(self.lib.asb_deflate_run_global(self.h, int(k0), int(k1)))

    def results(self, want_comps=True, want_weigs=True):
        K = self.K
        comps = np.empty((K, self.n_loc, 3)) if want_comps else None
        weigs = np.empty((self.F, K)) if want_weigs else None
        idx = np.empty(K, dtype=np.int64)
        sigma = np.empty(K)
        nr2 = np.empty(K)
        self._ck(self.lib.asb_deflate_results(self.h, ptr(comps), ptr(weigs), ptr(idx), ptr(sigma), ptr(nr2)))
        return dict(comps=comps, weigs=weigs, idx=idx, sigma=sigma, normR2_local=nr2)

    # ------------------------------------------------------------------ projection mode, panel steps
    NBINS = 2048

    def panel_scale(self, set_e0max=-1.0):
        a, b = ctypes.c_double(), ctypes.c_double()
        self._ck(self.lib.asb_panel_scale(self.h, ctypes.byref(a), ctypes.byref(b), float(set_e0max)))
        return a.value, b.value

    def panel_guess_stats(self):
        a, b, ok = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
        self._ck(self.lib.asb_panel_guess_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(ok)))
        return a.value, b.value, bool(ok.value)

    def panel_guess_begin(self, world):
        self._ck(self.lib.asb_panel_guess_begin(self.h, int(world)))

    def panel_guess_end(self):
        self._ck(self.lib.asb_panel_guess_end(self.h))

    def panel_hist(self, level, hist_ptr=None):
        self._ck(self.lib.asb_panel_hist(self.h, int(level), ctypes.c_void_p(hist_ptr) if hist_ptr else None))

    def panel_tau(self, level, hist_ptr=None):
        self._ck(self.lib.asb_panel_tau(self.h, int(level), ctypes.c_void_p(hist_ptr) if hist_ptr else None))

    def panel_top_energies(self, out_ptr, cap):
        self._ck(self.lib.asb_panel_top_energies(self.h, ctypes.c_void_p(out_ptr), int(cap)))

    def panel_global_tau(self, tab_ptr, world, cap):
        """Per-rank candidate counts after installing the global threshold; None when the table is too large for the
        device selection (the caller then selects with torch and calls panel_set_tau)."""
        counts = np.empty(world, dtype=np.int64)
        rc = self.lib.asb_panel_global_tau(self.h, ctypes.c_void_p(tab_ptr), int(world), int(cap), ptr(counts))
        if rc == _lib.ERR_LIMIT:
            return None
        self._ck(rc)
        return counts

    def panel_set_tau(self, tau_ptr):
        self._ck(self.lib.asb_panel_set_tau(self.h, ctypes.c_void_p(tau_ptr)))

    def panel_target(self):
        return int(self.lib.asb_panel_target(self.h))

    def panel_capacity(self):
        return int(self.lib.asb_panel_capacity(self.h))

    def panel_coop_possible(self):
        """Whether the co-resident panel kernel can run on this context (switched on and F <= 2048)."""
        return bool(self.lib.asb_panel_coop_possible(self.h))

    def panel_row_len(self):
        return 3 * ((self.F + 15) // 16 * 16)

    def panel_select(self, k, rows_ptr, idx_ptr, forced_gidx=-1, global_all=False, want_counts=True):
        if not want_counts:          # no host synchronisation: the caller knows the counts from the gathered energies
            self._ck(self.lib.asb_panel_select(self.h, int(k), int(forced_gidx), int(bool(global_all)),
                                               ctypes.c_void_p(rows_ptr), ctypes.c_void_p(idx_ptr), None, None))
            return None, None
        n, ov = ctypes.c_int64(), ctypes.c_int()
        self._ck(self.lib.asb_panel_select(self.h, int(k), int(forced_gidx), int(bool(global_all)),
                                           ctypes.c_void_p(rows_ptr), ctypes.c_void_p(idx_ptr), ctypes.byref(n),
                                           ctypes.byref(ov)))
        return n.value, bool(ov.value)

    def panel_assemble(self, rows_g_ptr, idx_g_ptr, counts, maxcount):
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        self._ck(self.lib.asb_panel_assemble(self.h, ctypes.c_void_p(rows_g_ptr), ctypes.c_void_p(idx_g_ptr), ptr(counts),
                                             int(counts.shape[0]), int(maxcount)))

    def panel_assemble_packed(self, packed_g_ptr, counts, maxcount):
        """One all-gathered buffer: per rank ``maxcount`` rows followed by ``maxcount`` vertex ids."""
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        self._ck(self.lib.asb_panel_assemble_packed(self.h, ctypes.c_void_p(packed_g_ptr), ptr(counts), int(counts.shape[0]),
                                                    int(maxcount)))

    def panel_run(self, k0, steps, global_all=False):
        c = ctypes.c_int64()
        self._ck(self.lib.asb_panel_run(self.h, int(k0), int(steps), int(bool(global_all)), 1, ctypes.byref(c)))
        return c.value

    def panel_project(self, k0, ncols):
        self._ck(self.lib.asb_panel_project(self.h, int(k0), int(ncols)))

    def panel_run_spec(self, k0, steps, global_all, spec_max):
        """panel_run that may append up to ``spec_max`` unproven steps: (steps run, provable head)."""
        ran, proven = ctypes.c_int64(), ctypes.c_int64()
        self._ck(self.lib.asb_panel_run_spec(self.h, int(k0), int(steps), int(bool(global_all)), 1, int(spec_max),
                                             ctypes.byref(ran), ctypes.byref(proven)))
        return ran.value, proven.value

    def panel_project_spec(self, k0, ncols, proven):
        """Pass over X for all ``ncols`` steps, energies untouched; first unproven step this shard rejects (ncols: none)."""
        r = ctypes.c_int64()
        self._ck(self.lib.asb_panel_project_spec(self.h, int(k0), int(ncols), int(proven), ctypes.byref(r)))
        return r.value

    def panel_project_spec_dev(self, k0, ncols, proven, out_dev_ptr):
        self._ck(self.lib.asb_panel_project_spec_dev(self.h, int(k0), int(ncols), int(proven), ctypes.c_void_p(out_dev_ptr)))

    def fetch_double(self, dev_ptr):
        v = ctypes.c_double()
        self._ck(self.lib.asb_fetch_double(self.h, ctypes.c_void_p(dev_ptr), ctypes.byref(v)))
        return v.value

    def fetch_doubles(self, dev_ptr, n):
        out = np.empty(int(n))
        self._ck(self.lib.asb_fetch_doubles(self.h, ctypes.c_void_p(dev_ptr), int(n), ptr(out)))
        return out

    def panel_read_run(self, k0, k1, nsub_max, spec_budget, sub_budget, words_dev_ptr):
        """All sub-panels of a multi-rank read in one launch, pass and tile checks behind it (asb.h: asb_panel_read_run):
        (ntile, [columns per tile], [provable head per tile]); the verdict words are left at words_dev_ptr (10 doubles)."""
        nt = ctypes.c_int(0)
        nc, pr = (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
        sb = (ctypes.c_int * 8)(*[int(x) for x in sub_budget])
        self._ck(self.lib.asb_panel_read_run(self.h, int(k0), int(k1), int(nsub_max), int(spec_budget), sb,
                                             ctypes.c_void_p(words_dev_ptr), ctypes.byref(nt), nc, pr))
        return nt.value, list(nc)[:nt.value], list(pr)[:nt.value]

    def panel_read_commit(self, words10):
        words10 = np.ascontiguousarray(words10, dtype=np.float64)
        assert words10.shape == (10,)
        tot, full, rej = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
        self._ck(self.lib.asb_panel_read_commit(self.h, ptr(words10), ctypes.byref(tot), ctypes.byref(full), ctypes.byref(rej)))
        return tot.value, full.value, bool(rej.value)

    def panel_set_coop(self, on):
        """Switches the co-resident panel kernel on / off; returns the previous setting."""
        return int(self.lib.asb_panel_set_coop(self.h, int(bool(on))))

    def panel_commit(self, k0, kept):
        self._ck(self.lib.asb_panel_commit(self.h, int(k0), int(kept)))

    def panel_refresh(self, k):
        e, g = ctypes.c_double(), ctypes.c_int64()
        self._ck(self.lib.asb_panel_refresh(self.h, int(k), ctypes.byref(e), ctypes.byref(g)))
        return e.value, g.value

    def deflate_stats(self):
        a, b = ctypes.c_int64(), ctypes.c_int64()
        self._ck(self.lib.asb_deflate_stats(self.h, ctypes.byref(a), ctypes.byref(b)))
        c, d = ctypes.c_int64(), ctypes.c_int64()
        self._ck(self.lib.asb_deflate_spec_stats(self.h, ctypes.byref(c), ctypes.byref(d)))
        e = ctypes.c_int64()
        self._ck(self.lib.asb_deflate_energy_passes(self.h, ctypes.byref(e)))
        f = ctypes.c_int64()
        self._ck(self.lib.asb_deflate_coop_fallbacks(self.h, ctypes.byref(f)))
        g = ctypes.c_int64()
        self._ck(self.lib.asb_deflate_guessed_panels(self.h, ctypes.byref(g)))
        h, i = ctypes.c_int64(), ctypes.c_int64()
        self._ck(self.lib.asb_deflate_sketch_stats(self.h, ctypes.byref(h), ctypes.byref(i)))
        j = ctypes.c_int64()
        self._ck(self.lib.asb_deflate_switch_stats(self.h, ctypes.byref(j)))
        l, m = ctypes.c_int64(), ctypes.c_int64()
        self._ck(self.lib.asb_deflate_read_stats(self.h, ctypes.byref(l), ctypes.byref(m)))
        return dict(panels=a.value, refreshes=b.value, unproven_tried=c.value, unproven_kept=d.value, energy_passes=e.value,
                    coop_fallbacks=f.value, guessed_panels=g.value, sketch_runs=h.value, sketch_reads=i.value,
                    residual_switch_at=j.value, coop_launches=l.value, max_read_kept=m.value)

    def project_switch_residual(self, k):
        """The run leaves the projection mode at component k and continues in the residual loop (asb.h)."""
        self._ck(self.lib.asb_project_switch_residual(self.h, int(k)))
        self.mode = _lib.DEFLATE_RESIDUAL

    def download_residual(self):
        out = np.empty((self.F, self.n_loc, 3))
        self._ck(self.lib.asb_deflate_download_residual(self.h, ptr(out)))
        return out

    # ------------------------------------------------------------------ reconstruction errors / held-out projection
    def recon_sweep(self, which, ks):
        """One read of the training (which 0) or held-out (1) tensor for all sweep points ``ks``: this shard's
        (S, 3) squared errors per axis, (S,) largest |error| and [sum T_x^2, sum T_y^2, sum T_z^2, max T]."""
        ks = np.ascontiguousarray(ks, dtype=np.int64)
        S = ks.shape[0]
        sums, mx, norms = np.empty((S, 3)), np.empty(S), np.empty(4)
        self._ck(self.lib.asb_recon_sweep(self.h, int(which), ptr(ks), S, ptr(sums), ptr(mx), ptr(norms)))
        return sums, mx, norms

    def heldout_upload(self, Y, massL, subtract, pre_scale_factor):
        """Y: host (F', N_glob, 3); this engine's vertex shard is taken from it and transformed like the training tensor."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        F, N, three = Y.shape
        assert three == 3
        if massL is not None:
            massL = np.ascontiguousarray(massL, dtype=np.float64)
            assert massL.shape == (N,)
        self._ck(self.lib.asb_heldout_upload(self.h, ptr(Y), F, N, self.v0, self.n_loc, ptr(massL), int(bool(subtract)),
                                             float(pre_scale_factor)))
        self.F_heldout = F

    def heldout_gram(self, P_dev_ptr=None, G_dev_ptr=None):
        self._ck(self.lib.asb_heldout_gram(self.h, ctypes.c_void_p(P_dev_ptr) if P_dev_ptr else None,
                                           ctypes.c_void_p(G_dev_ptr) if G_dev_ptr else None))

    def heldout_factor(self, P_dev_ptr=None, G_dev_ptr=None):
        n = ctypes.c_int64()
        self._ck(self.lib.asb_heldout_factor(self.h, ctypes.c_void_p(P_dev_ptr) if P_dev_ptr else None,
                                             ctypes.c_void_p(G_dev_ptr) if G_dev_ptr else None, ctypes.byref(n)))
        return n.value

    def heldout_weights(self):
        out = np.empty((self.F_heldout, self.K))
        self._ck(self.lib.asb_heldout_weights(self.h, ptr(out)))
        return out

    # ------------------------------------------------------------------ interpolation-error sweeps (constraint bases)
    def rows_gather(self, which, gidx):
        """Rows ``gidx`` (global) of the snapshots (which 0) or of the held-out frames (1) as (n, F, 3), and a bool mask of
        the rows this shard owns (the others are 0)."""
        gidx = np.ascontiguousarray(gidx, dtype=np.int64)
        n = gidx.shape[0]
        F = self.F if which == 0 else self.F_heldout
        out, owned = np.empty((n, F, 3)), np.empty(n, dtype=np.int32)
        self._ck(self.lib.asb_rows_gather(self.h, int(which), ptr(gidx), n, ptr(out), ptr(owned)))
        return out, owned.astype(bool)

    def interp_sweep(self, which, rp, npt, M, B):
        """One read of the tensor of ``which`` for the sweep points (rp[s], npt[s]); M: the concatenated (3, rp, npt)
        matrices, B: (nb, F, 3).  This shard's (S, 3) squared errors per axis, (S,) largest |error| and
        [sum f_x^2, sum f_y^2, sum f_z^2, max f]."""
        rp = np.ascontiguousarray(rp, dtype=np.int64)
        npt = np.ascontiguousarray(npt, dtype=np.int64)
        M = np.ascontiguousarray(M, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        S = rp.shape[0]
        sums, mx, norms = np.empty((S, 3)), np.empty(S), np.empty(4)
        self._ck(self.lib.asb_interp_sweep(self.h, int(which), ptr(rp), ptr(npt), S, ptr(M), ptr(B), B.shape[0], ptr(sums),
                                           ptr(mx), ptr(norms)))
        return sums, mx, norms

    # ------------------------------------------------------------------ on-mesh accuracy maps
    def onmesh_mesh(self, tris):
        """Uploads the triangles (M, 3) of the whole mesh with their vertex-star CSR (utils.vertex_star_csr); a repeated
        upload of the same triangles to this context is skipped."""
        from .utils import vertex_star_csr
        tris = np.ascontiguousarray(tris, dtype=np.int64)
        if tris.ndim != 2 or tris.shape[1] != 3:
            raise ValueError("triangles of shape %s: (M, 3) expected" % (tris.shape,))
        cached = getattr(self, "_onmesh_tris", None)
        if cached is not None and cached[0] == self.n_loc and np.array_equal(cached[1], tris):
            return
        self._onmesh_tris = None
        if tris.size and (tris.min() < 0 or tris.max() >= self.n_loc):
            raise ValueError("triangles name vertices outside 0..%d" % (self.n_loc - 1))
        sptr, star = vertex_star_csr(tris, self.n_loc)
        self._ck(self.lib.asb_onmesh_mesh(self.h, ptr(tris), tris.shape[0], ptr(sptr), ptr(star), self.v0, self.n_loc))
        self._onmesh_tris = (self.n_loc, tris.copy())

    def onmesh_run(self, which, r, f0, f1, fj, normals, inv_massL, add_mean, psf, denom, per_frame=False):
        """One r-component reconstruction of the training (which 0) or held-out (1) tensor over range(f0, f1, fj): this
        shard's dict of accum_norm (n_loc), mesh_num / mesh_den (F_sel), stats (10, see asb.h), with ``normals`` accum_angle
        (n_loc), with ``per_frame`` the (F_sel, n_loc) maps frame_err and angle."""
        n_sel = len(range(int(f0), int(f1), int(fj)))
        n = self.n_loc
        out = dict(accum_norm=np.empty(n), mesh_num=np.empty(n_sel), mesh_den=np.empty(n_sel), stats=np.empty(10))
        if normals:
            out["accum_angle"] = np.empty(n)
        if per_frame:
            out["frame_err"] = np.empty((n_sel, n))
            if normals:
                out["angle"] = np.empty((n_sel, n))
        inv_massL = self._invm(inv_massL)
        self._ck(self.lib.asb_onmesh_run(self.h, int(which), int(r), int(f0), int(f1), int(fj), int(bool(normals)),
                                         ptr(inv_massL), int(bool(add_mean)), float(psf), float(denom),
                                         ptr(out["accum_norm"]), ptr(out["mesh_num"]), ptr(out["mesh_den"]),
                                         ptr(out.get("accum_angle")), ptr(out["stats"]), ptr(out.get("frame_err")),
                                         ptr(out.get("angle"))))
        return out

    # ------------------------------------------------------------------ constraint projections of the resident positions
    def cproj_setup(self, setup):
        """Uploads one element kind (a ``projections.ProjectionSetup``); replaces the previous one of this context."""
        self._ck(self.lib.asb_cproj_setup(self.h, int(setup.code), int(setup.n_elem), ptr(setup.idx), ptr(setup.table),
                                          ptr(setup.star_ptr), ptr(setup.star_idx)))

    def cproj_run(self, which, f0, f1, fj, inv_massL, add_mean, psf, sigma_min, sigma_max, out_dev_ptr):
        """The projections of the frames range(f0, f1, fj) of the training (which 0) or held-out (1) tensor into the caller's
        device buffer of (F', rows, 3) float64."""
        inv_massL = self._invm(inv_massL)
        self._ck(self.lib.asb_cproj_run(self.h, int(which), int(f0), int(f1), int(fj), ptr(inv_massL), int(bool(add_mean)),
                                        float(psf), float(sigma_min), float(sigma_max), ctypes.c_void_p(int(out_dev_ptr))))

    def cforce_run(self, which, f0, f1, fj, inv_massL, add_mean, psf, sigma_min, sigma_max, St, accumulate, chunk_frames, out_dev_ptr):
        """The constraint forces S^T p of the same frames for the kind of the last ``cproj_setup`` into (or, ``accumulate``,
        onto) the caller's device buffer of (F', N, 3) float64.  ``St``: scipy CSR (N, rows) with sorted indices;
        ``chunk_frames``: frames per pass, 0 = automatic."""
        inv_massL = self._invm(inv_massL)
        n, indptr, indices, data = self._csr(St)
        self._ck(self.lib.asb_cforce_run(self.h, int(which), int(f0), int(f1), int(fj), ptr(inv_massL), int(bool(add_mean)),
                                         float(psf), float(sigma_min), float(sigma_max), n, ptr(indptr),
                                         ptr(indices), ptr(data), int(bool(accumulate)), int(chunk_frames),
                                         ctypes.c_void_p(int(out_dev_ptr))))

    # ------------------------------------------------------------------ DEIM-reduced constraint forces
    def rforce_operator(self, St, V):
        """M_d = S^T V_d on the device for ``St`` (scipy CSR (N, rows), sorted indices) and ``V`` (rows, mp, 3)."""
        V = np.ascontiguousarray(V, dtype=np.float64)
        assert V.ndim == 3 and V.shape[2] == 3
        n, indptr, indices, data = self._csr(St)
        self._ck(self.lib.asb_rforce_operator(self.h, n, ptr(indptr), ptr(indices), ptr(data), int(V.shape[0]),
                                              int(V.shape[1]), ptr(V)))

    def rforce_solver(self, H, rows):
        """``H`` (3, r, npt) and the rows of the sampled elements' stacked projections the npt interpolation points keep."""
        H = np.ascontiguousarray(H, dtype=np.float64)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        assert H.ndim == 3 and H.shape[0] == 3 and H.shape[2] == rows.shape[0]
        self._ck(self.lib.asb_rforce_solver(self.h, int(H.shape[1]), int(H.shape[2]), ptr(H), ptr(rows)))

    def rforce_bank(self, bank):
        """Selects which of the context's 8 banks ``rforce_operator``, ``rforce_solver``, ``rforce_run`` and ``hyper_operator``
        address from now on and a reduced ``pdsolve_slot`` binds; bank 0 is current in a new engine."""
        self._ck(self.lib.asb_rforce_bank(self.h, int(bank)))

    def rforce_run(self, which, f0, f1, fj, inv_massL, add_mean, psf, sigma_min, sigma_max, accumulate, out_dev_ptr):
        """The reduced constraint forces of the frames range(f0, f1, fj) into (or, ``accumulate``, onto) the caller's device
        buffer of (F', N, 3) float64; ``cproj_setup`` holds the sampled elements only."""
        inv_massL = self._invm(inv_massL)
        self._ck(self.lib.asb_rforce_run(self.h, int(which), int(f0), int(f1), int(fj), ptr(inv_massL), int(bool(add_mean)),
                                         float(psf), float(sigma_min), float(sigma_max), int(bool(accumulate)),
                                         ctypes.c_void_p(int(out_dev_ptr))))

    def force_diff(self, a_dev_ptr, b_dev_ptr, F, N, per_frame=False):
        """(3,) sum (a - b)^2 per axis, max |a - b|, [sum a_x^2, sum a_y^2, sum a_z^2, max a] and, ``per_frame``, the (F, 2)
        pairs [sum (a - b)^2, sum a^2] of two device tensors (F, N, 3)."""
        sums, mx, norms = np.empty(3), np.empty(1), np.empty(4)
        pf = np.empty((int(F), 2)) if per_frame else None
        self._ck(self.lib.asb_force_diff(self.h, ctypes.c_void_p(int(a_dev_ptr)), ctypes.c_void_p(int(b_dev_ptr)), int(F), int(N),
                                         ptr(sums), ptr(mx), ptr(norms), ptr(pf)))
        return sums, float(mx[0]), norms, pf

    # ------------------------------------------------------------------ global step of projective dynamics
    def gstep_setup(self, A):
        """Inverts ``A`` (scipy CSR (N, N), sorted indices, symmetric positive definite) on the device; the inverse stays with
        the context.  Returns max |A (A^-1 1) - 1|."""
        n, indptr, indices, data = self._csr(A)
        res = ctypes.c_double()
        self._gstep = self._gslab = self._gsub = None       # (the context holds one solver: the set-up releases the others)
        self._ck(self.lib.asb_gstep_setup(self.h, n, ptr(indptr), ptr(indices), ptr(data), ctypes.byref(res)))
        self._gstep = (indptr.copy(), indices.copy(), data.copy(), res.value)      # (copies: A stays the caller's)
        return res.value

    def gstep_held(self, A):
        """The residual of the last ``gstep_setup`` if its matrix was ``A`` entry for entry (the inverse is still on the device),
        else None."""
        held = getattr(self, "_gstep", None)
        if held is None or held[0].shape[0] != A.shape[0] + 1:
            return None
        same = all(np.array_equal(h, a) for h, a in zip(held[:3], (A.indptr, A.indices, A.data)))
        return held[3] if same else None

    def gstep_run(self, rhs_dev_ptr, n_frames, out_dev_ptr):
        """out = rhs A^-1 per coordinate on two device buffers of (n_frames, N, 3) float64 that do not overlap."""
        self._ck(self.lib.asb_gstep_run(self.h, ctypes.c_void_p(int(rhs_dev_ptr)), int(n_frames), ctypes.c_void_p(int(out_dev_ptr))))

    def gstep_inertia(self, which, f0, f1, fj, inv_massL, add_mean, psf, diag, mode, acc, rhs_dev_ptr):
        """rhs += diag * s for the frames range(f0, f1, fj): s = x + acc (``mode`` 0) or 2 x - x_prev + acc (1)."""
        inv_massL = self._invm(inv_massL)
        diag, acc = self._vec(diag, (self.N_glob,)), self._vec(acc, (3,))
        self._ck(self.lib.asb_gstep_inertia(self.h, int(which), int(f0), int(f1), int(fj), ptr(inv_massL), int(bool(add_mean)),
                                            float(psf), ptr(diag), int(mode), ptr(acc), ctypes.c_void_p(int(rhs_dev_ptr))))

    def gstep_inverse(self, n):
        """Test hook: the (n, n) inverse the context holds."""
        out = np.empty((int(n), int(n)))
        self._ck(self.lib.asb_test_gstep_inverse(self.h, ptr(out), int(n)))
        return out

    def gslab_setup(self, A, plan):
        """Factorises ``A`` (as ``gstep_setup`` takes it) block-tridiagonally over the slabs of ``plan``
        (``projections.slab_plan``) on the device; the factor replaces the explicit inverse in the context and every later
        ``gstep_run``, ``pdsolve_*`` and ``hyper_*`` call goes through it.  Returns (max |A (A^-1 1) - 1|, (slabs, largest
        padded slab))."""
        n, indptr, indices, data = self._csr(A)
        order = np.ascontiguousarray(plan.order, dtype=np.int64)
        sptr = np.ascontiguousarray(plan.slab_ptr, dtype=np.int64)
        res = ctypes.c_double()
        self._gstep = self._gslab = self._gsub = None
        self._ck(self.lib.asb_gslab_setup(self.h, n, ptr(indptr), ptr(indices), ptr(data), int(sptr.shape[0]) - 1, ptr(sptr),
                                          ptr(order), ctypes.byref(res)))
        info = self.gslab_info()
        self._gslab = (indptr.copy(), indices.copy(), data.copy(), order.copy(), sptr.copy(), res.value, (int(info[0]), int(info[1])))
        return res.value, self._gslab[6]

    def gslab_held(self, A, plan):
        """(residual, (slabs, largest padded slab)) of the last ``gslab_setup`` if its matrix and plan were these entry for
        entry (the factor is still on the device), else None."""
        held = getattr(self, "_gslab", None)
        if held is None or held[0].shape[0] != A.shape[0] + 1:
            return None
        same = all(np.array_equal(h, a) for h, a in zip(held[:5], (A.indptr, A.indices, A.data, plan.order, plan.slab_ptr)))
        return (held[5], held[6]) if same else None

    def gslab_info(self):
        """(slabs, largest padded slab, padded rows of the work matrix, doubles of the factor) of the factor on the device."""
        out = np.zeros(4, dtype=np.int64)
        self._ck(self.lib.asb_gslab_info(self.h, ptr(out)))
        return out

    def gslab_gemm_time(self, sp, w):
        """Timing hook: (ms of the sweep's product kernel, ms of asb_gemm_nn) on one (sp x sp)(sp x w) product, best of three."""
        out = np.zeros(2)
        self._ck(self.lib.asb_test_gslab_gemm_time(self.h, int(sp), int(w), ptr(out)))
        return float(out[0]), float(out[1])

    def gslab_solve(self, rhs):
        """Test hook: A^-1 ``rhs`` for a host array (N, w) through the device's sweep."""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        assert rhs.ndim == 2 and rhs.shape[0] == self.N_glob and rhs.shape[1] >= 1
        out = np.empty_like(rhs)
        self._ck(self.lib.asb_test_gslab_solve(self.h, ptr(rhs), int(rhs.shape[1]), ptr(out)))
        return out

    def gsub_setup(self, A, Qt, origin):
        """The position subspace q = o + U z as the global step's solver: ``A`` as ``gstep_setup`` takes it, ``Qt`` (3, r, N) the
        transposed basis per coordinate (``projections.subspace_basis``: orthonormal rows) and ``origin`` (N, 3).  The subspace
        replaces the explicit inverse or the slab factor in the context; every later ``gstep_run``, ``pdsolve_*`` and ``hyper_*``
        call applies o' + U (U^T A U)^-1 U^T rhs (``hyper_operator``: its linear part).  Returns max |U^T (A (P 1) - 1)|."""
        n, indptr, indices, data = self._csr(A)
        Qt = np.ascontiguousarray(Qt, dtype=np.float64)
        assert Qt.ndim == 3 and Qt.shape[0] == 3 and Qt.shape[2] == n
        origin = self._vec(origin, (n, 3))
        res = ctypes.c_double()
        self._gstep = self._gslab = self._gsub = None
        self._ck(self.lib.asb_gsub_setup(self.h, n, ptr(indptr), ptr(indices), ptr(data), int(Qt.shape[1]), ptr(Qt), ptr(origin),
                                         ctypes.byref(res)))
        self._gsub = (indptr.copy(), indices.copy(), data.copy(), Qt.copy(), origin.copy(), res.value)
        return res.value

    def gsub_held(self, A, Qt, origin):
        """The residual of the last ``gsub_setup`` if its matrix, basis and origin were these entry for entry (the subspace is
        still on the device), else None."""
        held = getattr(self, "_gsub", None)
        if held is None or held[0].shape[0] != A.shape[0] + 1:
            return None
        same = all(np.array_equal(h, a) for h, a in zip(held[:5], (A.indptr, A.indices, A.data, Qt, origin)))
        return held[5] if same else None

    def gsub_info(self):
        """(r, r rounded up to 16, N rounded up to 32, r rounded up to 4) of the subspace on the device."""
        out = np.zeros(4, dtype=np.int64)
        self._ck(self.lib.asb_gsub_info(self.h, ptr(out)))
        return out

    def gsub_apply(self, rhs, affine=True, out=None):
        """Test hook: o' + P ``rhs`` (``affine`` False: P ``rhs``) for a host array (3 N, w), row 3 v + d, through the device's
        two products.  Returns the whole (3 N, ld) matrix, ld = w rounded up to 64, as it came back: its columns past w are
        those of ``out`` (default NaN), which the device must not have written."""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        assert rhs.ndim == 2 and rhs.shape[0] == 3 * self.N_glob and rhs.shape[1] >= 1
        ld = (rhs.shape[1] + 63) // 64 * 64
        out = np.full((rhs.shape[0], ld), np.nan) if out is None else np.ascontiguousarray(out, dtype=np.float64)
        assert out.shape == (rhs.shape[0], ld)
        self._ck(self.lib.asb_test_gsub_apply(self.h, ptr(rhs), int(rhs.shape[1]), int(bool(affine)), ptr(out)))
        return out

    def gsub_state(self):
        """Test hook: what ``gsub_setup`` left -- ``(W, Ainv, origin', Ut)``: W_d = (U_d^T A U_d)^-1 U_d^T (3, r, N), the inverses
        (3, r, r), o' (N, 3) and the basis as uploaded (3, r, N), without their padding."""
        r, rq, Np, rp = (int(x) for x in self.gsub_info())
        n = self.N_glob
        raw = []
        for which, shape in enumerate(((3, Np, rq), (3, rq, rq), (n, 3), (3, rp, Np))):
            a = np.empty(shape)
            self._ck(self.lib.asb_test_gsub_state(self.h, which, ptr(a), int(a.size)))
            raw.append(a)
        return (np.ascontiguousarray(raw[0][:, :n, :r].transpose(0, 2, 1)), raw[1][:, :r, :r].copy(), raw[2], raw[3][:, :r, :n].copy())

    # ------------------------------------------------------------------ roll-outs with the state in z (csrc/asb_zroll.hip)
    def gsub_coordinates(self, which, f0, f1, fj, inv_massL, add_mean, psf, out_dev_ptr, pos_dev_ptr=None, n_frames=0):
        """z = U^T (x - o) of the frames range(f0, f1, fj) of the tensor ``which`` -- or of the caller's device tensor
        (``n_frames``, N, 3) -- into the caller's device buffer of (F', r, 3) float64."""
        inv_massL = self._invm(inv_massL)
        self._ck(self.lib.asb_gsub_coordinates(self.h, int(which), int(f0), int(f1), int(fj), ptr(inv_massL), int(bool(add_mean)), float(psf),
                                               ctypes.c_void_p(int(pos_dev_ptr)) if pos_dev_ptr else None, int(n_frames),
                                               ctypes.c_void_p(int(out_dev_ptr))))

    def gsub_expand(self, z_dev_ptr, n_frames, out_dev_ptr):
        """o + U z of the caller's (``n_frames``, r, 3) into the caller's device buffer of (``n_frames``, N, 3) float64."""
        self._ck(self.lib.asb_gsub_expand(self.h, ctypes.c_void_p(int(z_dev_ptr)), int(n_frames), ctypes.c_void_p(int(out_dev_ptr))))

    def gsub_expand_diff(self, a_dev_ptr, z_dev_ptr, n_frames, per_frame=False):
        """What ``force_diff(a, o + U z)`` returns for the caller's device tensors ``a`` (``n_frames``, N, 3) and ``z``
        (``n_frames``, r, 3), with o + U z formed and consumed in one kernel and never stored."""
        sums, mx, norms = np.empty(3), np.empty(1), np.empty(4)
        pf = np.empty((int(n_frames), 2)) if per_frame else None
        self._ck(self.lib.asb_gsub_expand_diff(self.h, ctypes.c_void_p(int(a_dev_ptr)), ctypes.c_void_p(int(z_dev_ptr)), int(n_frames),
                                               ptr(sums), ptr(mx), ptr(norms), ptr(pf)))
        return sums, float(mx[0]), norms, pf

    def zroll_operator(self):
        """(U^T A U)^-1 U^T S^T V of the current bank from the subspace of ``gsub_setup`` and the operator of ``rforce_operator``;
        either call afterwards invalidates it."""
        self._ck(self.lib.asb_zroll_operator(self.h))

    def zroll_begin(self, which, f0, f1, fj, inv_massL, add_mean, psf, diag, mode, acc, touched, z_dev_ptr=None, zprev_dev_ptr=None):
        """Begins a roll-out in z over the frames range(f0, f1, fj): T, kappa, the ``touched`` rows of U and the state -- the
        projections of the frames (``mode`` 1: z_prev from the previous frame, 0: z_prev = z) or the caller's pair (F', r, 3)."""
        inv_massL = self._invm(inv_massL)
        diag, acc = self._vec(diag, (self.N_glob,)), self._vec(acc, (3,))
        touched = np.ascontiguousarray(touched, dtype=np.int64)
        assert touched.ndim == 1
        self._ck(self.lib.asb_zroll_begin(self.h, int(which), int(f0), int(f1), int(fj), ptr(inv_massL), int(bool(add_mean)), float(psf),
                                          ptr(diag), int(mode), ptr(acc), int(touched.shape[0]), ptr(touched),
                                          ctypes.c_void_p(int(z_dev_ptr)) if z_dev_ptr else None,
                                          ctypes.c_void_p(int(zprev_dev_ptr)) if zprev_dev_ptr else None))

    def zroll_slot(self, sigma_min, sigma_max):
        """The kind of the last ``cproj_setup`` (numbered in the touched vertices) becomes the next reduced kind of the roll-out."""
        self._ck(self.lib.asb_zroll_slot(self.h, float(sigma_min), float(sigma_max)))

    def zroll_pins(self, row0=0):
        """Binds the pins of ``pins_set`` to the roll-out in z: step t from frame f reads row ``row0`` + f + t - 1 of the shift."""
        self._ck(self.lib.asb_zroll_pins(self.h, int(row0)))

    def zroll_forces(self, row0=0):
        """Binds the force table of ``ext_set`` (no floor) to the roll-out in z: step t from frame f reads row ``row0`` + f + t - 1."""
        self._ck(self.lib.asb_zroll_forces(self.h, int(row0)))

    def zroll_steps(self, n_steps, n_iter, chunk_frames=0, record_every=0, records_dev_ptr=None):
        """``n_steps`` time steps of ``n_iter`` iterations in stream order, one drain at the end; ``record_every`` > 0: z after
        every such step into the caller's device buffer (R, F', r, 3)."""
        self._ck(self.lib.asb_zroll_steps(self.h, int(n_steps), int(n_iter), int(chunk_frames), int(record_every),
                                          ctypes.c_void_p(int(records_dev_ptr)) if records_dev_ptr else None))

    def zroll_state(self, z_dev_ptr, zprev_dev_ptr):
        """z and z_prev of the roll-out into the caller's two device buffers of (F', r, 3) float64."""
        self._ck(self.lib.asb_zroll_state(self.h, ctypes.c_void_p(int(z_dev_ptr)), ctypes.c_void_p(int(zprev_dev_ptr))))

    def zroll_affine(self, Ms, Xs, base):
        """Test hook: base + sum_s Ms[s] @ Xs[s] per coordinate through the product kernel alone.  ``Ms[s]`` (3, r, k_s), ``Xs[s]``
        (3, k_s, w), ``base`` (3, r, w) or (3, r) (broadcast).  Returns the whole padded (3, rq, ld) result."""
        Ms = [np.ascontiguousarray(M, dtype=np.float64) for M in Ms]
        Xs = [np.ascontiguousarray(X, dtype=np.float64) for X in Xs]
        base = np.ascontiguousarray(base, dtype=np.float64)
        r, w = Ms[0].shape[1], Xs[0].shape[2]
        assert all(M.shape[:2] == (3, r) and X.shape == (3, M.shape[2], w) for M, X in zip(Ms, Xs)) and base.shape in ((3, r), (3, r, w))
        klen = np.array([M.shape[2] for M in Ms], dtype=np.int64)
        Mh = np.concatenate([M.ravel() for M in Ms])
        Xh = np.concatenate([X.ravel() for X in Xs])
        out = np.empty((3, (r + 15) // 16 * 16, (w + 63) // 64 * 64))
        self._ck(self.lib.asb_test_zroll_affine(self.h, r, w, len(Ms), ptr(klen), ptr(Mh), ptr(Xh), ptr(base), int(base.ndim == 2), ptr(out)))
        return out

    # ------------------------------------------------------------------ solver iterations of projective dynamics
    def pdsolve_begin(self, which, f0, f1, fj, inv_massL, add_mean, psf, diag, mode, acc, start, start_dev_ptr=None):
        """Begins a solve over the frames range(f0, f1, fj) after ``gstep_setup``: the inertia term diag * s (``mode``, ``acc`` as
        ``gstep_inertia``) and the iterate, started at s (``start`` 0), at the frame (1) or at the caller's device buffer of
        (F', N, 3) float64 (2)."""
        inv_massL = self._invm(inv_massL)
        diag, acc = self._vec(diag, (self.N_glob,)), self._vec(acc, (3,))
        self._pd_frames = None
        self._ck(self.lib.asb_pdsolve_begin(self.h, int(which), int(f0), int(f1), int(fj), ptr(inv_massL), int(bool(add_mean)),
                                            float(psf), ptr(diag), int(mode), ptr(acc), int(start),
                                            ctypes.c_void_p(int(start_dev_ptr)) if start_dev_ptr else None))
        self._pd_frames = len(range(int(f0), int(f1), int(fj)))

    def pdsolve_slot(self, sigma_min, sigma_max, St=None):
        """The kind of the last ``cproj_setup`` becomes the next term of the solve in progress, with ``St`` (scipy CSR (N, rows),
        sorted indices); ``St`` None: the reduced term of the sampled elements with the engine's operator and solver."""
        if St is None:
            self._ck(self.lib.asb_pdsolve_slot(self.h, float(sigma_min), float(sigma_max), 1, 0, None, None, None))
            return
        n, indptr, indices, data = self._csr(St)
        self._ck(self.lib.asb_pdsolve_slot(self.h, float(sigma_min), float(sigma_max), 0, n, ptr(indptr), ptr(indices),
                                           ptr(data)))

    def pdsolve_iterate(self, n_iter, chunk_frames=0, out_dev_ptr=None, history=False):
        """``n_iter`` iterations of the solve in progress; the last iterate into the caller's device buffer of (F', N, 3) float64
        if given.  ``history``: returns the (n_iter, F', 2) array [|q_new - q_old|^2, |q_new|^2], else None."""
        frames = getattr(self, "_pd_frames", None)
        hist = np.empty((max(int(n_iter), 0), frames, 2)) if history and frames is not None else None
        self._ck(self.lib.asb_pdsolve_iterate(self.h, int(n_iter), int(chunk_frames),
                                              ctypes.c_void_p(int(out_dev_ptr)) if out_dev_ptr else None, ptr(hist)))
        return hist

    def hyper_operator(self):
        """G_d = A^-1 (S^T V_d) on the device from the inverse of ``gstep_setup`` and the operator of ``rforce_operator``; either
        call afterwards invalidates it."""
        self._ck(self.lib.asb_hyper_operator(self.h))

    def hyper_iterate(self, n_iter, touched=None, chunk_frames=0, out_dev_ptr=None):
        """``n_iter`` hyper-reduced iterations of the solve in progress, whose slots are all reduced kinds, each on its own bank
        (``rforce_bank``).  ``touched``: the ascending vertices every slot's set-up is renumbered into -- the union over the kinds
        (all but the last iteration run on those rows) --, or None: the set-ups name the mesh's vertices and every iteration runs
        on all rows."""
        if touched is not None:
            touched = np.ascontiguousarray(touched, dtype=np.int64)
            assert touched.ndim == 1
        self._ck(self.lib.asb_hyper_iterate(self.h, int(n_iter), 0 if touched is None else int(touched.shape[0]), ptr(touched),
                                            int(chunk_frames), ctypes.c_void_p(int(out_dev_ptr)) if out_dev_ptr else None))

    # ------------------------------------------------------------------ time steps on the solve's state
    def pdsolve_carry(self, pos_dev_ptr=None):
        """The solve in progress gets the positions at the start of its time step: the begun frames x_f, or the caller's
        device buffer of (F', N, 3) float64."""
        self._ck(self.lib.asb_pdsolve_carry(self.h, ctypes.c_void_p(int(pos_dev_ptr)) if pos_dev_ptr else None))

    def pdsolve_advance(self):
        """The end of a time step: with q the iterate and p the carried positions, s = 2 q - p + acc becomes the iterate and
        the explicit state of the inertia term, q the carried positions.  In stream order; does not wait."""
        self._ck(self.lib.asb_pdsolve_advance(self.h))

    def pdsolve_positions(self, out_dev_ptr):
        """The carried positions into the caller's device buffer of (F', N, 3) float64."""
        self._ck(self.lib.asb_pdsolve_positions(self.h, ctypes.c_void_p(int(out_dev_ptr))))

    def pdsolve_state(self, which):
        """Test hook: the iterate (``which`` 0) or the carried positions (1) as stored, (3 N, F' rounded up to 64)."""
        ld = (self._pd_frames + 63) // 64 * 64
        out = np.empty((3 * self.N_glob, ld))
        self._ck(self.lib.asb_test_pdsolve_state(self.h, int(which), ptr(out), out.shape[0], ld))
        return out

    # ------------------------------------------------------------------ positional constraints (pins)
    def pins_set(self, vertices, wi, p0, shift=None):
        """The pins of every later ``pins_term`` / ``pdsolve_pins``: ``vertices`` (P,) of the resident tensor, no two equal,
        ``wi`` (P,) >= 0, ``p0`` (P, 3), ``shift`` None, (T_s, 3) or (T_s, P, 3); checked and uploaded once."""
        v = np.ascontiguousarray(vertices, dtype=np.int64)
        P = int(v.shape[0])
        wi, p0 = self._vec(wi, (P,)), self._vec(p0, (P, 3))
        if shift is not None:
            shift = np.ascontiguousarray(shift, dtype=np.float64)
            assert shift.shape[1:] in ((3,), (P, 3))
        self._ck(self.lib.asb_pins_set(self.h, P, ptr(v), ptr(wi), ptr(p0), 0 if shift is None else int(shift.shape[0]), ptr(shift),
                                       int(shift is not None and shift.ndim == 3)))

    def pins_clear(self):
        self._ck(self.lib.asb_pins_clear(self.h))

    def pins_term(self, f0, f1, fj, row0, accumulate, out_dev_ptr):
        """The pin term wi (p0 + shift[row0 + f]) of the frames range(f0, f1, fj) into (``accumulate``: onto the pinned entries
        of) the caller's device buffer of (F', N, 3) float64."""
        self._ck(self.lib.asb_pins_term(self.h, int(f0), int(f1), int(fj), int(row0), int(bool(accumulate)), ctypes.c_void_p(int(out_dev_ptr))))

    def fm_add(self, a_dev_ptr, b_dev_ptr, length):
        """a += b on two device buffers of ``length`` float64 that do not overlap: the add of a solver iteration."""
        self._ck(self.lib.asb_fm_add(self.h, ctypes.c_void_p(int(a_dev_ptr)), ctypes.c_void_p(int(b_dev_ptr)), int(length)))

    def pdsolve_pins(self, row0=0):
        """Binds the pins of ``pins_set`` to the solve in progress: their term joins the inertia term, frame f with row
        ``row0`` + f of the shift, and every later ``pdsolve_advance`` renews it one row further."""
        self._ck(self.lib.asb_pdsolve_pins(self.h, int(row0)))

    # ------------------------------------------------------------------ external forces and the floor
    def ext_set(self, table=None, floor=None):
        """The forces and the floor of every later ``pdsolve_external``: ``table`` None, (3 N,) (a constant force) or (T_s, 3 N),
        the displacements dt^2 force / mass; ``floor`` None or (height, axis); checked and uploaded once."""
        if table is not None:
            table = np.ascontiguousarray(table, dtype=np.float64)
        h, axis = (0.0, 1) if floor is None else floor
        self._ck(self.lib.asb_ext_set(self.h, 0 if table is None or table.ndim == 1 else int(table.shape[0]), ptr(table),
                                      int(floor is not None), int(axis), float(h)))

    def ext_clear(self):
        self._ck(self.lib.asb_ext_clear(self.h))

    def pdsolve_external(self, row0=0):
        """Binds the forces and the floor of ``ext_set`` to the solve in progress, before ``pdsolve_pins``: the explicit state of
        frame f takes row ``row0`` + f of the table and is clamped to the floor, the inertia term is rewritten, and every later
        ``pdsolve_advance`` does both in its own pass, one row further."""
        self._ck(self.lib.asb_pdsolve_external(self.h, int(row0)))

    # ------------------------------------------------------------------ SPLOCS
    def splocs_begin(self):
        self._ck(self.lib.asb_splocs_begin(self.h))

    def splocs_gram(self, P_dev_ptr=None, M_dev_ptr=None, want_norm=False):
        nx = ctypes.c_double()
        self._ck(self.lib.asb_splocs_gram(self.h, ctypes.c_void_p(P_dev_ptr) if P_dev_ptr else None,
                                          ctypes.c_void_p(M_dev_ptr) if M_dev_ptr else None,
                                          ctypes.byref(nx) if want_norm else None))
        return nx.value if want_norm else None

    def splocs_weights(self, P_dev_ptr=None, M_dev_ptr=None):
        idx = np.empty(self.K, dtype=np.int64)
        val = np.empty(self.K)
        self._ck(self.lib.asb_splocs_weights(self.h, ctypes.c_void_p(P_dev_ptr) if P_dev_ptr else None,
                                             ctypes.c_void_p(M_dev_ptr) if M_dev_ptr else None, ptr(idx), ptr(val)))
        return idx, val

    def splocs_trace_begin(self, n_its):
        self._ck(self.lib.asb_splocs_trace_begin(self.h, int(n_its)))

    def splocs_objective_dev(self, it, P_dev_ptr=None, M_dev_ptr=None):
        self._ck(self.lib.asb_splocs_objective_dev(self.h, ctypes.c_void_p(P_dev_ptr) if P_dev_ptr else None,
                                                   ctypes.c_void_p(M_dev_ptr) if M_dev_ptr else None, int(it)))

    def splocs_trace(self, n_its):
        out = np.empty((int(n_its), 3))
        self._ck(self.lib.asb_splocs_trace(self.h, int(n_its), ptr(out)))
        return out

    def splocs_admm(self, Lambda_loc, rho, n_iter):
        Lambda_loc = np.ascontiguousarray(Lambda_loc, dtype=np.float64)
        assert Lambda_loc.shape == (self.K, self.n_loc)
        self._ck(self.lib.asb_splocs_admm(self.h, ptr(Lambda_loc), float(rho), int(n_iter)))

    def splocs_admm_fields(self, slots, lam, dmin, dmax, rho, n_iter):
        """ADMM step with Lambda built on the device from cached distance fields (geodesic_cache_add)."""
        slots = np.ascontiguousarray(slots, dtype=np.int64)
        assert slots.shape == (self.K,)
        self._ck(self.lib.asb_splocs_admm_fields(self.h, ptr(slots), float(lam), float(dmin), float(dmax), float(rho), int(n_iter)))

    def splocs_objective(self, P_dev_ptr=None, M_dev_ptr=None):
        wp, gm, sp = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        self._ck(self.lib.asb_splocs_objective(self.h, ctypes.c_void_p(P_dev_ptr) if P_dev_ptr else None,
                                               ctypes.c_void_p(M_dev_ptr) if M_dev_ptr else None, ctypes.byref(wp),
                                               ctypes.byref(gm), ctypes.byref(sp)))
        return wp.value, gm.value, sp.value

    def splocs_results(self):
        C = np.empty((self.K, self.n_loc, 3))
        W = np.empty((self.F, self.K))
        self._ck(self.lib.asb_splocs_results(self.h, ptr(C), ptr(W)))
        return C, W

    # ------------------------------------------------------------------ post-processing
    # ------------------------------------------------------------------ device geodesics
    def geodesic_setup(self, heat, lap, grad, div, dense=False, coarse=None, slabs=None):
        """heat, lap, grad, div: scipy CSR matrices (float64).  dense: invert the two SPD systems explicitly on the
        device (asb_geodesic_dense_setup) instead of solving them by PCG per batch.  coarse = (agg, heat_c, lap_c): the
        aggregates and dense coarse operators of the PCG mode's two-level preconditioner."""
        keep = []

        def csr(m):
            m = m.tocsr()
            m.sum_duplicates()
            m.sort_indices()
            rp, ci, v = m.indptr.astype(np.int32), m.indices.astype(np.int32), np.ascontiguousarray(m.data, dtype=np.float64)
            keep.extend([rp, ci, v])
            return [rp.ctypes.data, ci.ctypes.data, v.ctypes.data]

        n, m3 = heat.shape[0], grad.shape[0]
        dh = np.ascontiguousarray(heat.diagonal(), dtype=np.float64)
        dl = np.ascontiguousarray(lap.diagonal(), dtype=np.float64)
        args = csr(heat) + csr(lap) + csr(grad) + csr(div) + [dh.ctypes.data, dl.ctypes.data]
        self._ck(self.lib.asb_geodesic_setup(self.h, int(n), int(m3), *args))
        self._geo_n = n
        self.geodesic_dense = bool(dense) or slabs is not None      # (the whole local step can stay on the device)
        if slabs is not None:
            # slab mode: order (permuted index -> vertex), ptr (slab boundaries); both matrices go over in the permuted numbering
            order, ptr_ = slabs
            order = np.ascontiguousarray(order, dtype=np.int64)
            inv = np.empty(n, dtype=np.int32)
            inv[order] = np.arange(n, dtype=np.int32)
            hp = heat.tocsr()[order][:, order]
            lp = lap.tocsr()[order][:, order]
            ptr32 = np.ascontiguousarray(ptr_, dtype=np.int32)
            self._ck(self.lib.asb_geodesic_bt_setup(self.h, int(ptr32.shape[0] - 1), ptr32.ctypes.data, inv.ctypes.data,
                                                    *(csr(hp) + csr(lp))))
        elif dense:
            self._ck(self.lib.asb_geodesic_dense_setup(self.h))
        elif coarse is not None:
            agg, heat_c, lap_c, omega = coarse
            agg = np.ascontiguousarray(agg, dtype=np.int32)
            nc = int(agg.max()) + 1
            order = np.argsort(agg, kind="stable").astype(np.int32)
            ptr_ = np.zeros(nc + 1, dtype=np.int32)
            np.cumsum(np.bincount(agg, minlength=nc), out=ptr_[1:])
            heat_c = np.ascontiguousarray(heat_c, dtype=np.float64)
            lap_c = np.ascontiguousarray(lap_c, dtype=np.float64)
            assert heat_c.shape == lap_c.shape == (nc, nc) and agg.shape == (n,)
            self._ck(self.lib.asb_geodesic_coarse_setup(self.h, nc, agg.ctypes.data, ptr_.ctypes.data, order.ctypes.data,
                                                        heat_c.ctypes.data, lap_c.ctypes.data, float(omega)))

    def apply_geodesic(self, k, dmin, dmax):
        self._ck(self.lib.asb_deflate_apply_geodesic(self.h, int(k), float(dmin), float(dmax)))

    GEODESIC_CACHE_SLOTS = 64 * 64

    def geodesic_cache_add(self, sources, tol=1e-13):
        """Solves the distance fields of ``sources`` and keeps them on the device; returns their cache slots."""
        src = np.ascontiguousarray(sources, dtype=np.int64)
        slots = []
        for b in range(0, src.shape[0], 64):
            part = src[b:b + 64]
            s0 = ctypes.c_int64()
            self._ck(self.lib.asb_geodesic_cache_add(self.h, ptr(part), int(part.shape[0]), float(tol), ctypes.addressof(s0)))
            slots.extend(range(s0.value, s0.value + part.shape[0]))
        return slots

    def geodesic_cache_clear(self):
        self._ck(self.lib.asb_geodesic_cache_clear(self.h))

    def geodesic_solve(self, sources, tol=1e-13):
        src = np.ascontiguousarray(sources, dtype=np.int64)
        out = np.empty((src.shape[0], self._geo_n))
        it = (ctypes.c_int * 2)()
        self._ck(self.lib.asb_geodesic_solve(self.h, ptr(src), int(src.shape[0]), float(tol), ptr(out), it))
        return out, (it[0], it[1])

    # ------------------------------------------------------------------ ingest
    def align_frames(self, frames, rigid=True):
        """Rigid Procrustes alignment of every frame to frame 0; returns (aligned (F,N,3) f64, T (F,4,4))."""
        fr = np.array(frames, dtype=np.float64, order="C", copy=True)
        T = np.empty((fr.shape[0], 4, 4))
        self._ck(self.lib.asb_align_frames(self.h, ptr(fr), fr.shape[0], fr.shape[1], int(bool(rigid)), ptr(T)))
        return fr, T

    # ------------------------------------------------------------------ POD / QR / DEIM (config 5)
    def pod_gram(self, G_dev_ptr=None, to_host=True):
        G = np.empty((self.F, self.F)) if to_host else None
        self._ck(self.lib.asb_pod_gram(self.h, ctypes.c_void_p(G_dev_ptr) if G_dev_ptr else None, ptr(G)))
        return G

    def pod_basis(self, V, sigma):
        V = np.ascontiguousarray(V, dtype=np.float64)
        sigma = np.ascontiguousarray(sigma, dtype=np.float64)
        assert V.shape == (self.F, sigma.shape[0])
        self._ck(self.lib.asb_pod_basis(self.h, ptr(V), ptr(sigma), sigma.shape[0]))
        self.K = int(sigma.shape[0])

    def pod_project(self, B_dev_ptr=None, to_host=True):
        B = np.empty((self.K, self.F)) if to_host else None
        self._ck(self.lib.asb_pod_project(self.h, ctypes.c_void_p(B_dev_ptr) if B_dev_ptr else None, ptr(B)))
        return B

    def sym_tridiag(self, n, A_dev_ptr=None):
        """Householder tridiagonalisation of the n x n symmetric device matrix (default: the POD Gram matrix)."""
        d, e = np.empty(n), np.empty(max(n - 1, 0))
        self._ck(self.lib.asb_sym_tridiag(self.h, ctypes.c_void_p(A_dev_ptr) if A_dev_ptr else None, int(n), ptr(d),
                                          ptr(e) if n > 1 else ptr(np.empty(1))))
        return d, e

    def sym_backtransform(self, n, Z, A_dev_ptr=None):
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        assert Z.shape[0] == n
        V = np.empty_like(Z)
        self._ck(self.lib.asb_sym_backtransform(self.h, ctypes.c_void_p(A_dev_ptr) if A_dev_ptr else None, int(n), ptr(Z),
                                                int(Z.shape[1]), ptr(V)))
        return V

    def sym_eig_topk(self, n, k, A_dev_ptr=None, want_vectors=False):
        """All eigenvalues (descending) of the n x n symmetric device matrix (default: the POD Gram matrix) and its k
        leading eigenvectors, entirely on the device; the vectors stay there for ``pod_basis_dev``."""
        lam = np.empty(n)
        V = np.empty((n, k)) if want_vectors else None
        bad = ctypes.c_int64()
        self._ck(self.lib.asb_sym_eig_topk(self.h, ctypes.c_void_p(A_dev_ptr) if A_dev_ptr else None, int(n), int(k), ptr(lam),
                                           ptr(V), ctypes.byref(bad)))
        return (lam, V, bad.value) if want_vectors else (lam, bad.value)

    def pod_basis_dev(self, K):
        self._ck(self.lib.asb_pod_basis_dev(self.h, int(K)))
        self.K = int(K)

    def pod_slices(self, p, K):
        self._ck(self.lib.asb_pod_slices(self.h, int(p), int(K)))
        self.K = int(K)

    def pod_slice_grams(self, p, s0, ns, G_dev_ptr):
        """Partial Gram matrices of slices s0 .. s0 + ns - 1 over this shard into the device buffer (ns x F x F)."""
        self._ck(self.lib.asb_pod_slice_grams(self.h, int(p), int(s0), int(ns), ctypes.c_void_p(G_dev_ptr)))

    def pod_slice_eig(self, K, G_dev_ptr, VS_dev_ptr, status_dev_ptr):
        """One slice's eigen-solve: V S^-1 (F x K) and the refusal flag into device exchange slots."""
        self._ck(self.lib.asb_pod_slice_eig(self.h, int(K), ctypes.c_void_p(G_dev_ptr), ctypes.c_void_p(VS_dev_ptr),
                                            ctypes.c_void_p(status_dev_ptr)))

    def pod_slices_basis(self, p, K, VS_all_dev_ptr):
        """This shard's basis rows from every slice's V S^-1 (the all-reduced exchange buffer)."""
        self._ck(self.lib.asb_pod_slices_basis(self.h, int(p), int(K), ctypes.c_void_p(VS_all_dev_ptr)))
        self.K = int(K)

    def pod_rotate(self, B_dev_ptr=None):
        S = np.empty(self.K)
        self._ck(self.lib.asb_pod_rotate(self.h, ctypes.c_void_p(B_dev_ptr) if B_dev_ptr else None, ptr(S)))
        return S

    def pod_deflate_begin(self, keep, B_dev_ptr=None):
        self._ck(self.lib.asb_pod_deflate_begin(self.h, ctypes.c_void_p(B_dev_ptr) if B_dev_ptr else None, int(keep)))

    def pod_deflate_end(self, last, K_total):
        self._ck(self.lib.asb_pod_deflate_end(self.h, int(last)))
        self.K = int(K_total)

    def pod_power(self, B_dev_ptr=None):
        self._ck(self.lib.asb_pod_power(self.h, ctypes.c_void_p(B_dev_ptr) if B_dev_ptr else None))

    def qr_apply_joint(self, G_dev_ptr=None):
        self._ck(self.lib.asb_qr_apply_joint(self.h, ctypes.c_void_p(G_dev_ptr) if G_dev_ptr else None))

    # host-array probes of the small dense device solvers (tests)
    def test_tridiag_eig(self, d, e, k):
        d = np.ascontiguousarray(d, dtype=np.float64)
        e = np.ascontiguousarray(e, dtype=np.float64)
        n = d.shape[0]
        lam, Z, bad = np.empty(n), np.empty((n, max(k, 1))), ctypes.c_int64()
        self._ck(self.lib.asb_test_tridiag_eig(self.h, ptr(d), ptr(e) if n > 1 else ptr(np.zeros(1)), n, int(k), ptr(lam),
                                               ptr(Z), ctypes.byref(bad)))
        return lam, Z[:, :k], bad.value

    def test_jacobi_rows(self, A, want_u=True):
        A = np.ascontiguousarray(A, dtype=np.float64)
        nv, m = A.shape
        U = np.empty((nv, nv)) if want_u else None
        sig, sw = np.empty(nv), ctypes.c_int64()
        self._ck(self.lib.asb_test_jacobi_rows(self.h, ptr(A), nv, m, ptr(U), ptr(sig), ctypes.byref(sw)))
        return U, sig, sw.value

    def test_project_columns(self, W, k0, ncols, out, col_scale=None, path=0):
        """out[:ncols] = X . W[:, k0:k0 + ncols] / col_scale[k0:k0 + ncols] through the 16-column (path 0) or the multi-tile
        (path 1) projection kernels; W (F, ldw); out (out_cols, 3 n_loc) is updated in place, all of it round-trips."""
        W = np.ascontiguousarray(W, dtype=np.float64)
        assert W.ndim == 2 and W.shape[0] == self.F
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.shape[1] == 3 * self.n_loc
        if col_scale is not None:
            col_scale = np.ascontiguousarray(col_scale, dtype=np.float64)
            assert col_scale.shape == (W.shape[1],)
        self._ck(self.lib.asb_test_project_columns(self.h, ptr(W), W.shape[1], int(k0), int(ncols), ptr(col_scale), int(path),
                                                   ptr(out), out.shape[0]))
        return out

    # the dense f64 building blocks on host arrays (tests/test_gpu_dense_blocks.py); outputs are updated in place, all of them
    def test_gemm_nn(self, A, B, C, ldc, M, N, Kc, alpha=1.0, beta=0.0, tri=0):
        """C (1-D, rows of stride ldc) = beta C + alpha A[:M, :Kc] B[:Kc, :N] through asb_gemm_nn; A, B 2-D contiguous (their
        widths are the strides); all of C round-trips."""
        for a in (A, B, C):
            assert a.dtype == np.float64 and a.flags.c_contiguous
        assert A.ndim == 2 and B.ndim == 2 and C.ndim == 1
        self._ck(self.lib.asb_test_gemm_nn(self.h, ptr(A), A.shape[1], ptr(B), B.shape[1], ptr(C), int(ldc), int(M), int(N), int(Kc),
                                           float(alpha), float(beta), int(tri), C.size))
        return C

    def test_gemm_tn(self, form, X, R, I, J, out, Y=None, sx=1, so_i=None, so_j=1, I_split=0):
        """form 0: out.flat[i so_i + j so_j] = sum_r X[r, i sx] Y[r, j] (so_i defaults to J); 1: out[:I*J] = X[:, :I]^T Y[:, :J];
        2: out[:I*I] = X[:, :I]^T X[:, :I].  X (R, ldx), Y (R, ldy) 2-D contiguous; out 1-D, all of it round-trips."""
        assert X.dtype == np.float64 and X.flags.c_contiguous and X.shape[0] == R
        assert out.dtype == np.float64 and out.flags.c_contiguous and out.ndim == 1
        if Y is not None:
            assert Y.dtype == np.float64 and Y.flags.c_contiguous and Y.shape[0] == R
        self._ck(self.lib.asb_test_gemm_tn(self.h, int(form), ptr(X), X.shape[1], int(sx), ptr(Y), Y.shape[1] if Y is not None else 0,
                                           int(R), int(I), int(J), ptr(out), int(J if so_i is None else so_i), int(so_j), out.size,
                                           int(I_split)))
        return out

    def test_transpose(self, A, out):
        A = np.ascontiguousarray(A, dtype=np.float64)
        assert out.dtype == np.float64 and out.flags.c_contiguous
        self._ck(self.lib.asb_test_transpose(self.h, ptr(A), A.shape[0], A.shape[1], ptr(out), out.size))
        return out

    def test_sym_eig(self, A):
        """(lam descending, V with eigenvectors as columns, status word) of the one-block Jacobi solver (n <= 128)."""
        A = np.ascontiguousarray(A, dtype=np.float64)
        n = A.shape[0]
        lam, V, st = np.empty(n), np.empty((n, n)), ctypes.c_int()
        self._ck(self.lib.asb_test_sym_eig(self.h, ptr(A), n, ptr(lam), ptr(V), ctypes.byref(st)))
        return lam, V, st.value

    def test_spd_inverse(self, A):
        A = np.ascontiguousarray(A, dtype=np.float64)
        out = np.empty_like(A)
        self._ck(self.lib.asb_test_spd_inverse(self.h, ptr(A), A.shape[0], ptr(out)))
        return out

    def test_chol_tinv(self, G):
        G = np.ascontiguousarray(G, dtype=np.float64)
        Tt = np.empty_like(G)
        self._ck(self.lib.asb_test_chol_tinv(self.h, ptr(G), G.shape[0], ptr(Tt)))
        return Tt

    # the greedy step of the residual mode, one piece at a time (tests/test_gpu_deflate_step.py)
    def test_eig3_dev(self, A6, fast, slack=8):
        """(n, 4) rows (lambda, u) of eig3_top (fast=False) / eig3_top_fast (True) run on the device on A6 (n, 6); `slack` doubles
        behind the result round-trip too and are asserted untouched."""
        A6 = np.ascontiguousarray(A6, dtype=np.float64)
        n = A6.shape[0]
        out = np.full(4 * n + slack, -7.25)
        self._ck(self.lib.asb_test_eig3_dev(self.h, int(bool(fast)), ptr(A6), n, ptr(out), out.size))
        assert (out[4 * n:] == -7.25).all(), "asb_test_eig3_dev wrote behind its result"
        return out[:4 * n].reshape(n, 4)

    def test_cproj_project_dev(self, kind, mats, sigma_min, sigma_max, slack=8):
        """"Project F" of one element kind (projections.KINDS code 1, 2 or 3) on the device, one thread per matrix: mats (n, 2, 2)
        or (n, 3, 3) -> the n projections of the same shape; `slack` doubles behind the result are asserted untouched."""
        mats = np.ascontiguousarray(mats, dtype=np.float64)
        n, w = mats.shape[0], mats[0].size
        out = np.full(w * n + slack, -7.25)
        self._ck(self.lib.asb_test_cproj_project_dev(self.h, int(kind), ptr(mats), n, float(sigma_min), float(sigma_max), ptr(out),
                                                     out.size))
        assert (out[w * n:] == -7.25).all(), "asb_test_cproj_project_dev wrote behind its result"
        return out[:w * n].reshape(mats.shape)

    def test_deflate_step(self, k, w, wn2, s_loc=None):
        w = np.ascontiguousarray(w, dtype=np.float64)
        assert w.shape == (self.F,)
        if s_loc is not None:
            s_loc = np.ascontiguousarray(s_loc, dtype=np.float64)
            assert s_loc.shape == (self.n_loc,)
        self._ck(self.lib.asb_test_deflate_step(self.h, int(k), ptr(w), float(wn2), ptr(s_loc)))

    def test_deflate_state(self, want_R=False, want_W=False):
        """dict: energy (n_loc), pmax / pidx / psum (nblk), nblk, nblk_cap, scal (K + 1, 4; column 2 holds index bits) and, on
        request, W (K, Fp) and R (n_loc, 3, Fp) with their padding."""
        cnt = np.zeros(2, dtype=np.int64)
        self._ck(self.lib.asb_test_deflate_state(self.h, None, None, None, None, ptr(cnt), None, None, None))
        nblk, cap = int(cnt[0]), int(cnt[1])
        Fp = (self.F + 15) // 16 * 16
        energy, scal = np.empty(self.n_loc), np.empty((self.K + 1, 4))
        pmax, psum, pidx = np.empty(nblk), np.empty(nblk), np.empty(nblk, dtype=np.int64)
        W = np.empty((self.K, Fp)) if want_W else None
        R = np.empty((self.n_loc, 3, Fp)) if want_R else None
        self._ck(self.lib.asb_test_deflate_state(self.h, ptr(energy), ptr(pmax), ptr(pidx), ptr(psum), None, ptr(scal), ptr(W),
                                                 ptr(R)))
        return dict(energy=energy, pmax=pmax, pidx=pidx, psum=psum, nblk=nblk, nblk_cap=cap, scal=scal, W=W, R=R)

    def test_prep_state(self, want_X=False, want_energies=True):
        """dict of what the snapshot preparation left (tests/test_gpu_prep.py): flags e0_valid / ev_valid / have_mean; on request
        X (n_loc, 3, Fp) with its padding; with want_energies (after `scale`) E0, EV (n_loc), sc (the six device scalars |X|^2,
        max E0, sum m_v, -, sum EV, sum EV^2) and the host fields ev_cv2, mean_frac, mean_energy, prep_normx2.  The energies are
        those of the last scaling sweep: they describe the current tensor only while e0_valid / ev_valid are set."""
        Fp = (self.F + 15) // 16 * 16
        X = np.empty((self.n_loc, 3, Fp)) if want_X else None
        E0 = np.empty(self.n_loc) if want_energies else None
        EV = np.empty(self.n_loc) if want_energies else None
        sc = np.empty(10) if want_energies else None
        flags = np.zeros(3, dtype=np.int32)
        self._ck(self.lib.asb_test_prep_state(self.h, ptr(X), ptr(E0), ptr(EV), ptr(sc), ptr(flags)))
        out = dict(X=X, E0=E0, EV=EV, e0_valid=bool(flags[0]), ev_valid=bool(flags[1]), have_mean=bool(flags[2]))
        if want_energies:
            out.update(sc=sc[:6].copy(), ev_cv2=float(sc[6]), mean_frac=float(sc[7]), mean_energy=float(sc[8]),
                       prep_normx2=float(sc[9]))
        return out

    def test_local_best(self, k):
        rec = np.empty(self.xchg_len())
        self._ck(self.lib.asb_test_local_best(self.h, int(k), ptr(rec)))
        return rec

    def test_pick_records(self, k, recs):
        recs = np.ascontiguousarray(recs, dtype=np.float64)
        assert recs.ndim == 2 and recs.shape[1] == self.xchg_len()
        self._ck(self.lib.asb_test_pick_records(self.h, int(k), ptr(recs), recs.shape[0]))

    # the SPLOCS state between two phases (tests/test_gpu_splocs_phases.py), after splocs_begin
    def test_splocs_install(self, C=None, W=None, U=None):
        """Overwrites the SPLOCS state: C (K, n_loc, 3), W (F, K), U (K, n_loc, 3); None leaves a piece as it is."""
        arrs = []
        for a, shape in ((C, (self.K, self.n_loc, 3)), (W, (self.F, self.K)), (U, (self.K, self.n_loc, 3))):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64)
                assert a.shape == shape, (a.shape, shape)
            arrs.append(a)
        self._ck(self.lib.asb_test_splocs_install(self.h, ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2])))

    def test_splocs_state(self):
        """dict: U (K, n_loc, 3), Lambda (K, n_loc), G and Ginv (K, K), c (K, 3 n_loc) as the last phase left them."""
        K, n = self.K, self.n_loc
        out = dict(U=np.empty((K, n, 3)), Lambda=np.empty((K, n)), G=np.empty((K, K)), Ginv=np.empty((K, K)), c=np.empty((K, 3 * n)))
        self._ck(self.lib.asb_test_splocs_state(self.h, ptr(out["U"]), ptr(out["Lambda"]), ptr(out["G"]), ptr(out["Ginv"]),
                                                ptr(out["c"])))
        return out

    # the device geodesics on small meshes (tests/test_gpu_geodesic_small.py); none of these changes the solver's state
    def test_slab_gemm64(self, A, Z, out, Kc, alpha=1.0, beta=0.0, nct=4):
        """out (M, 64) = beta out + alpha A[:, :Kc] Z (Kc, 64) through slab_gemm64, in place; A (M, lda) 2-D contiguous."""
        for a in (A, Z, out):
            assert a.dtype == np.float64 and a.flags.c_contiguous and a.ndim == 2
        assert Z.shape == (Kc, 64) and out.shape == (A.shape[0], 64)
        self._ck(self.lib.asb_test_slab_gemm64(self.h, ptr(A), A.shape[1], ptr(Z), ptr(out), A.shape[0], int(Kc), float(alpha),
                                               float(beta), int(nct)))
        return out

    def test_geodesic_field1(self, src):
        """(n,) the distance field apply_geodesic solves for its source, for a source given here."""
        phi = np.empty(self._geo_n)
        self._ck(self.lib.asb_test_geodesic_field1(self.h, int(src), ptr(phi)))
        return phi

    def test_support_weights(self, phi, v0, n_loc, dmin, dmax):
        phi = np.ascontiguousarray(phi, dtype=np.float64)
        s = np.empty(max(int(n_loc), 0))
        self._ck(self.lib.asb_test_support_weights(self.h, ptr(phi), phi.shape[0], int(v0), int(n_loc), float(dmin), float(dmax),
                                                   ptr(s)))
        return s

    def test_geodesic_cached(self, slot):
        out = np.empty(self._geo_n)
        self._ck(self.lib.asb_test_geodesic_cached(self.h, int(slot), ptr(out)))
        return out

    def snapshots_affine(self, inv_scale, add_mean, rowscale_loc=None):
        if rowscale_loc is not None:
            rowscale_loc = np.ascontiguousarray(rowscale_loc, dtype=np.float64)
        self._ck(self.lib.asb_snapshots_affine(self.h, float(inv_scale), int(bool(add_mean)), ptr(rowscale_loc)))

    def qr_apply(self, G_dev_ptr=None):
        self._ck(self.lib.asb_qr_apply(self.h, ctypes.c_void_p(G_dev_ptr) if G_dev_ptr else None))

    def deim_step(self, k, coef=None):
        if coef is not None:
            coef = np.ascontiguousarray(coef, dtype=np.float64)
            assert coef.shape == (3, k)
        i, v = ctypes.c_int64(), ctypes.c_double()
        self._ck(self.lib.asb_deim_step(self.h, int(k), ptr(coef), ctypes.byref(i), ctypes.byref(v)))
        return i.value, v.value

    def deim_run(self):
        """The whole DEIM loop on the device (single rank): (Pt (K,), maxabs (K,), solve_failed); None when K is too large
        for the solve kernel's LDS (nothing was launched: the caller runs the host loop)."""
        Pt, ma, bad = np.empty(self.K, dtype=np.int64), np.empty(self.K), ctypes.c_int()
        rc = self.lib.asb_deim_run(self.h, Pt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ptr(ma), ctypes.byref(bad))
        if rc == _lib.ERR_LIMIT:
            return None
        self._ck(rc)
        return Pt, ma, bad.value

    def deim_block_step(self, k, p, coef, group):
        """Residual of basis block k (p vectors) and its arg-max over rows (group = 1) or constraints (group = p):
        (index, energy, largest |r|)."""
        if coef is not None:
            coef = np.ascontiguousarray(coef, dtype=np.float64)
            assert coef.shape == (3, k * p, p)
        am, idx, val = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        self._ck(self.lib.asb_deim_block_residual(self.h, int(k), int(p), ptr(coef), ctypes.byref(am)))
        self._ck(self.lib.asb_energy_block_argmax(self.h, int(group), ctypes.byref(idx), ctypes.byref(val)))
        return idx.value, val.value, am.value

    def st_upload(self, St):
        """The sparse differential operator S^T (scipy sparse, |V| x e p) as CSR on the device."""
        St = St.tocsr()
        St.sort_indices()
        n, indptr, indices, data = self._csr(St)
        self._ck(self.lib.asb_st_upload(self.h, n, int(St.shape[1]), int(data.shape[0]), ptr(indptr),
                                        ptr(indices), ptr(data)))

    def st_residual_argmax(self):
        v, val = ctypes.c_int64(), ctypes.c_double()
        self._ck(self.lib.asb_st_residual_argmax(self.h, ctypes.byref(v), ctypes.byref(val)))
        return v.value, val.value

    def residual_norm2(self):
        out = ctypes.c_double()
        self._ck(self.lib.asb_deflate_residual_norm2(self.h, ctypes.byref(out)))
        return out.value

    def deim_block_step_st(self, k, p, coef):
        """Residual of basis block k mapped to position space by S^T: (vertex arg-max, its energy, largest |r|)."""
        if coef is not None:
            coef = np.ascontiguousarray(coef, dtype=np.float64)
            assert coef.shape == (3, k * p, p)
        am, v, val = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        self._ck(self.lib.asb_deim_block_residual_st(self.h, int(k), int(p), ptr(coef), ctypes.byref(am), ctypes.byref(v),
                                                     ctypes.byref(val)))
        return v.value, val.value, am.value

    # ---- S^T with the constraint rows sharded over several ranks (asb.h: asb_st_upload_shard ...)
    def st_upload_shard(self, indptr, slots, data, n_halo):
        """CSR of the position vertices this rank owns, columns as local slots (< n_loc: this shard, then the halo)."""
        indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        slots = np.ascontiguousarray(slots, dtype=np.int64)
        data = np.ascontiguousarray(data, dtype=np.float64)
        self._ck(self.lib.asb_st_upload_shard(self.h, int(indptr.shape[0] - 1), int(data.shape[0]), ptr(indptr), ptr(slots),
                                              ptr(data), int(n_halo)))

    def st_halo_pack(self, which, gidx, out_dev_ptr):
        gidx = np.ascontiguousarray(gidx, dtype=np.int64)
        self._ck(self.lib.asb_st_halo_pack(self.h, int(which), ptr(gidx), int(gidx.shape[0]), ctypes.c_void_p(out_dev_ptr)))

    def st_halo_fill(self, which, src_dev_ptr, slot, n_src):
        slot = np.ascontiguousarray(slot, dtype=np.int64)
        self._ck(self.lib.asb_st_halo_fill(self.h, int(which), ctypes.c_void_p(src_dev_ptr), ptr(slot), int(n_src)))

    def st_halo_deflate(self, k):
        self._ck(self.lib.asb_st_halo_deflate(self.h, int(k)))

    def st_shard_residual_argmax(self):
        """(index into the owned vertices or -1, energy)"""
        v, val = ctypes.c_int64(), ctypes.c_double()
        self._ck(self.lib.asb_st_shard_residual_argmax(self.h, ctypes.byref(v), ctypes.byref(val)))
        return v.value, val.value

    def deim_block_step_st_shard(self, k, p, coef):
        """deim_block_step_st over the owned vertices: (index into them or -1, its energy, largest |r| of their rows)."""
        if coef is not None:
            coef = np.ascontiguousarray(coef, dtype=np.float64)
            assert coef.shape == (3, k * p, p)
        am, v, val = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
        self._ck(self.lib.asb_deim_block_residual_st_shard(self.h, int(k), int(p), ptr(coef), ctypes.byref(am), ctypes.byref(v),
                                                           ctypes.byref(val)))
        return v.value, val.value, am.value

    def st_shard_stats(self):
        """dict(halo, owned, nnz, basis_K)"""
        out = np.zeros(4, dtype=np.int64)
        self._ck(self.lib.asb_st_shard_stats(self.h, ptr(out)))
        return dict(halo=int(out[0]), owned=int(out[1]), nnz=int(out[2]), basis_K=int(out[3]))

    def st_halo_download(self, which):
        """The halo copies: which 0 (h, 3, F) residual rows, 1 (K, h, 3) basis rows."""
        st = self.st_shard_stats()
        out = np.empty((st["halo"], 3, self.F)) if which == 0 else np.empty((st["basis_K"], st["halo"], 3))
        self._ck(self.lib.asb_st_halo_download(self.h, int(which), ptr(out)))
        return out

    def deim_row(self, gidx):
        row = np.empty((self.K, 3))
        rc = self.lib.asb_deim_row(self.h, int(gidx), ptr(row))
        if rc == 1:
            return None
        self._ck(rc)
        return row

    def components_stream(self, enable=True):
        """Overlapped download of the basis into pinned host memory (asb.h: asb_components_stream_into).  The buffer belongs
        to THIS object and to the ndarrays ``components_pinned`` returns, not to the context: switching the stream off,
        closing the engine or starting another run never frees or overwrites memory a live ndarray looks at."""
        self._streaming = bool(enable)
        if not enable:
            self._ck(self.lib.asb_components_stream_into(self.h, None, 0))
            self._pin = None

    def components_pinned(self):
        """(K, n_loc, 3) ndarray over the pinned buffer the run streamed its basis into.  Safe to keep: the memory lives as
        long as the array (or any view of it) does, and a later run on this engine takes a fresh buffer while it is alive."""
        pin = getattr(self, "_pin", None)
        if not getattr(self, "_streaming", False) or pin is None:
            raise RuntimeError("components_pinned: components_stream(True) was not on when the run began")
        p = ctypes.c_void_p()
        self._ck(self.lib.asb_components_pinned(self.h, ctypes.byref(p)))
        assert p.value == pin.ptr
        return pin.view((int(self.K), int(self.n_loc), 3))

    def deflate_reserve(self, K_new):
        """Residual mode: room for K_new components in all, keeping what the run has produced (asb.h: asb_deflate_reserve)."""
        self._ck(self.lib.asb_deflate_reserve(self.h, int(K_new)))
        self.K = max(int(self.K), int(K_new))

    def results_comps(self):
        out = np.empty((self.K, self.n_loc, 3))
        self._ck(self.lib.asb_components_download(self.h, ptr(out)))
        return out

    def components_expand(self, coef):
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        assert coef.ndim == 3 and coef.shape[0] == 3
        out = np.empty((coef.shape[2], self.n_loc, 3))
        self._ck(self.lib.asb_components_expand(self.h, ptr(coef), coef.shape[1], coef.shape[2], ptr(out)))
        return out

    def components_truncate(self, K):
        self._ck(self.lib.asb_components_truncate(self.h, int(K)))
        self.K = int(K)

    def components_upload(self, comps_loc):
        comps_loc = np.ascontiguousarray(comps_loc, dtype=np.float64)
        assert comps_loc.ndim == 3 and comps_loc.shape[1:] == (self.n_loc, 3)
        self._ck(self.lib.asb_components_upload(self.h, ptr(comps_loc), comps_loc.shape[0]))
        self.K = int(comps_loc.shape[0])

    def orth_gram(self, G_dev_ptr=None):
        self._ck(self.lib.asb_orth_gram(self.h, ctypes.c_void_p(G_dev_ptr) if G_dev_ptr else None))

    def orth_apply(self, G_dev_ptr=None):
        sing = np.empty((3, self.K))
        self._ck(self.lib.asb_orth_apply(self.h, ctypes.c_void_p(G_dev_ptr) if G_dev_ptr else None, ptr(sing)))
        return sing

    def orth_gram_get(self):
        G = np.empty((3, self.K, self.K))
        self._ck(self.lib.asb_orth_gram_get(self.h, ptr(G)))
        return G

    def components_transform(self, T):
        T = np.ascontiguousarray(T, dtype=np.float64)
        assert T.shape == (3, self.K, self.K)
        self._ck(self.lib.asb_components_transform(self.h, ptr(T)))

    def orth_refine(self, G_dev_ptr=None):
        self._ck(self.lib.asb_orth_refine(self.h, ctypes.c_void_p(G_dev_ptr) if G_dev_ptr else None))

    def components_post(self, unscale, pre_scale_factor, invMassL_loc=None, download=True):
        """``download=False``: the basis stays on the device (a later step changes or reads it there): no 8 K n_loc 3 bytes
        through a pageable buffer (config 5: 307 MB, 25 ms)."""
        out = np.empty((self.K, self.n_loc, 3)) if download else None
        if invMassL_loc is not None:
            invMassL_loc = np.ascontiguousarray(invMassL_loc, dtype=np.float64)
        self._ck(self.lib.asb_components_post(self.h, int(bool(unscale)), float(pre_scale_factor), ptr(invMassL_loc),
                                              ptr(out)))
        return out
