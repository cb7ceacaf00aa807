"""``posComponents`` -- drop-in mirror of the reference class (snapbases/posComponents.py)
for the snapshot-reduction hot path, computing on the MI355X through ``libasb_hip.so``.

Same constructor (``posComponents(param)``), attribute and method names as the reference
(:19-49 and the methods listed in SURVEY.md 8b).  ``param`` is any object exposing the
attributes of the reference's ``Config_parameters`` that this path reads.

There is no CPU path: without the HIP library / a gfx950 GPU construction fails.
"""
import csv
import os

import numpy as np
from numpy import maximum, clip, sqrt, errstate, newaxis, empty, eye, allclose, dot, zeros, tensordot
from scipy.linalg import norm, svd, orth

from . import _lib
from .distributed import Comm
from .posSnapshots import posSnapshots
from . import utils as _u
from ._panels import deflate_panels_multirank
from .utils import log_time, store_components, testSparsity, test_linear_dependency


SMALL_TENSOR_BYTES = 256 << 20
SWEEP_POINTS_PER_READ = 1024      # asb_recon_sweep: sweep points per read of the tensor


def n_loc_of(snaps):
    return snaps._shards[snaps._comm.rank][1]


def _auto_global_mode(F, n_loc, multi):
    """Which device algorithm for support='global'.  The panel (projection) algorithm wins as soon as a read of X costs
    more than its per-panel overheads; a shard that fits the 256 MB Infinity Cache together with its residual copy
    (bunny: 68 MB) is faster through the plain residual loop, which has no host round trip at all (measured at
    14 290 x 200, K = 32: 1.3 ms against 2.8 ms).  Several ranks always use the panel protocol."""
    Fp = (int(F) + 15) // 16 * 16
    return "residual" if (not multi and 24 * int(n_loc) * Fp <= SMALL_TENSOR_BYTES) else "project"


class posComponents:  # Components == bases
    def __init__(self, param, pos_snapshots=None):
        self.basesType = param.vertPos_bases_type
        assert self.basesType == 'PCA' or self.basesType == 'SPLOCS'

        if pos_snapshots is None:
            train = os.path.join(param.aligned_snapshots_directory, param.train_aligned_snapshots_animation_file)
            test = os.path.join(param.aligned_snapshots_directory, param.test_aligned_snapshots_animation_file)
            pos_snapshots = posSnapshots(train, test, param.vertPos_rest_shape, param.vertPos_masses_file,
                                         param.tet_mesh_file, param.q_standarize, param.q_massWeight)
        self.pos_snapshots = pos_snapshots

        self.numComp = param.vertPos_numComponents
        self.support = param.q_support              # 'local' | 'global'
        self.storeSingVal = param.store_vertPos_PCA_sing_val

        self._comps = None            # host copy (cache of the device-resident basis, or user-assigned)
        self._comps_on_device = False  # True: the authoritative (K, n_loc, 3) basis is in HBM
        self._comps_post_processed = False     # True once post_process_components has un-scaled the basis
        self.weigs = None
        self.ortho_comps = None
        self.smooth_min_dist = param.vertPos_smooth_min_dist
        self.smooth_max_dist = param.vertPos_smooth_max_dist
        self.output_components_file = "components.h5"

        self.measures_at_largeDeforVerts = None
        self.fileNameBases = "q_pos_"
        self.param = param

        # extras (not in the reference): the selected vertices; which device algorithm to use
        # (None = automatic, "residual", "project"; env ASB_DEFLATE_MODE overrides the default)
        self.selected_vertices = None
        self.deflate_mode = os.environ.get("ASB_DEFLATE_MODE") or None
        self._stepwise_panels = False      # tests: drive the multi-rank panel protocol on one rank

    # ------------------------------------------------------------------ comps: device-resident, lazy download
    @property
    def comps(self):
        if self._comps is None and self._comps_on_device:
            eng, comm = self.pos_snapshots._engine, self.pos_snapshots._comm
            if getattr(self, "_comps_streamed", False) and getattr(eng, "_streaming", False) and not comm.multi:
                # the engine streamed the rows into its pinned buffer while it computed (HipEngine.components_stream): a plain
                # ndarray over that buffer, valid until the next run on this engine (np.array(...) to keep it longer)
                self._comps = eng.components_pinned()
                return self._comps
            loc = eng.results(want_comps=True, want_weigs=False)["comps"]
            self._comps = comm.all_gather_rows(loc, self.pos_snapshots.nVerts, axis=1)
        return self._comps

    @comps.setter
    def comps(self, value):
        self._comps = value
        self._comps_on_device = False
        self._comps_post_processed = False

    # ------------------------------------------------------------------ statics (same as the reference)
    @staticmethod
    def project_weight(x):
        """posComponents.py:52-58."""
        x = maximum(0., x)
        max_x = x.max()
        if max_x == 0:
            return x
        else:
            return x / max_x

    @staticmethod
    def compute_support_map(idx, geodesics, min_dist, max_dist):
        """posComponents.py:61-64."""
        phi = geodesics(idx)
        return (clip(phi, min_dist, max_dist) - min_dist) / (max_dist - min_dist)

    @staticmethod
    def prox_l1l2(Lambda, x, beta):
        """posComponents.py:252-256."""
        xlen = sqrt((x ** 2).sum(axis=-1))
        with errstate(divide='ignore'):
            shrinkage = maximum(0.0, 1 - beta * Lambda / xlen)
        return x * shrinkage[..., newaxis]

    # ------------------------------------------------------------------ the hot path
    @log_time("")
    def extract_k_components(self, writer, num_iters_max=20, num_admm_iterations=10):
        """posComponents.py:67-129 on the GPU.

        support='global' on one rank runs all K components back to back on the device;
        support='local' (host geodesic support map between select and apply) and multi-rank
        runs step through select -> [all-gather] -> pick -> apply per component.
        """
        snaps = self.pos_snapshots
        eng, comm = snaps._engine, snaps._comm
        K = self.numComp
        local = self.support == 'local'
        if local and snaps.compute_geodesic_distance is None:
            raise ValueError("support='local' needs the mesh triangles (geodesic support maps)")
        # global support on one rank: residual-free panel algorithm (one read of X per panel of up to
        # 16 components); otherwise the residual tensor is kept and updated per component.
        mode = self.deflate_mode
        if mode is None:
            mode = "residual" if local else _auto_global_mode(self.pos_snapshots.frs, n_loc_of(snaps), comm.multi)
        if mode == "project" and local:
            raise ValueError("deflate_mode='project' needs global support")
        eng.deflate_begin(K, local, _lib.DEFLATE_PROJECT if mode == "project" else _lib.DEFLATE_RESIDUAL)
        v0, n_loc = snaps._shards[comm.rank]

        if not comm.multi and not local and not self._stepwise_panels:
            eng.run_global(0, K)
        elif mode == "project":
            self._project_multirank(K)
        else:
            rec = recs = None
            if comm.multi:
                rec, recs = comm.new_records(eng.xchg_len(), eng.device_exchange)
            geo = snaps.compute_geodesic_distance
            if local and hasattr(geo, "prepare"):
                geo.prepare()                         # (lazy: built on first use, posSnapshots only records mesh and backend)
            on_device_maps = local and getattr(geo, "_engine", None) is eng and getattr(eng, "geodesic_dense", False) \
                and type(self).compute_support_map is posComponents.compute_support_map
            for k in range(K):
                if comm.multi:
                    eng.local_best(k, rec.data_ptr())
                    comm.all_gather_records(rec, recs)
                    eng.pick(k, recs.data_ptr(), comm.world)
                else:
                    eng.pick(k)
                s_loc = None
                if local and on_device_maps:          # pick -> distance field -> support weights -> pass: no host round trip
                    eng.apply_geodesic(k, self.smooth_min_dist, self.smooth_max_dist)
                    continue
                if local:
                    idx, _ = eng.get_pick(k)
                    s = 1 - self.compute_support_map(idx, snaps.compute_geodesic_distance,
                                                     self.smooth_min_dist, self.smooth_max_dist)      # (N,)
                    s_loc = s[v0:v0 + n_loc]
                eng.apply(k, s_loc)

        res = eng.results(want_comps=False, want_weigs=True)
        normR = np.sqrt(np.maximum(comm.allreduce_sum(res["normR2_local"]), 0.0))     # |X|^2 - sum can round below 0 once |R| < 1e-8 |X|
        self.weigs = res["weigs"]
        self.selected_vertices = res["idx"]
        self._comps, self._comps_on_device = None, True
        self._comps_streamed = True     # the engine's pinned buffer (if it streams) holds exactly this run's basis
        self.measures_at_largeDeforVerts = np.column_stack([np.arange(K, dtype=np.float64), res["sigma"], normR])
        if self.storeSingVal and writer is not None:
            for k in range(K):
                writer.writerow([k, float(res["sigma"][k]), float(normR[k])])

        if self.basesType == 'SPLOCS':
            self.splocs_glob_optimization(self.param.splocs_max_itrs, self.param.splocs_admm_num_itrs,
                                          None, snaps.compute_geodesic_distance)
        print("Computed '", self.basesType, "' bases size ", (K, snaps.nVerts, 3))

    def _project_multirank(self, K):
        snaps = self.pos_snapshots
        deflate_panels_multirank(snaps._engine, snaps._comm, snaps.nVerts, K)

    @log_time("")
    def splocs_glob_optimization(self, num_iters_max, num_admm_iterations, R, compute_geodesic_distance):
        with _u.no_gc():          # (a garbage collection inside the loop is 2 - 3 ms of idle GPU: utils.no_gc)
            return self._splocs_glob_optimization(num_iters_max, num_admm_iterations, R, compute_geodesic_distance)

    def _splocs_glob_optimization(self, num_iters_max, num_admm_iterations, R, compute_geodesic_distance):
        """posComponents.py:131-189 on the GPU (csrc/asb_splocs.hip).

        Like the reference, this leaves ``comps`` / ``weigs`` untouched (the reference works on
        local copies and discards them) and prints one
        ``itr %03d, Energy =%f, Error =%f`` line per outer iteration.  Extras: the refined
        ``splocs_comps`` (K,N,3), ``splocs_weigs`` (F,K), ``splocs_trace`` (its,2) and
        ``splocs_centres`` (its,K) attributes.  ``R`` is accepted for signature compatibility;
        the device works from X, W and C (the residual is never formed).
        """
        snaps = self.pos_snapshots
        eng, comm = snaps._engine, snaps._comm
        K, N, F = self.numComp, snaps.nVerts, snaps.frs
        v0, n_loc = snaps._shards[comm.rank]
        lam, rho = self.param.splocs_lambda, self.param.splocs_rho
        if compute_geodesic_distance is None:
            raise ValueError("SPLOCS needs the mesh triangles (geodesic support maps)")
        eng.splocs_begin()
        Pbuf = Mbuf = None
        if comm.multi:
            Pbuf, Mbuf = comm.new_gram_buffers(F, K, eng.device_exchange)

        def gram(want_norm=False):
            nx = eng.splocs_gram(Pbuf.data_ptr() if Pbuf is not None else None,
                                 Mbuf.data_ptr() if Mbuf is not None else None, want_norm)
            if comm.multi:                 # partial Gram matrices: RCCL all-reduce (sum) over the ranks
                comm.allreduce_tensor(Pbuf)
                comm.allreduce_tensor(Mbuf)
            return nx

        def ptrs():
            return (Pbuf.data_ptr(), Mbuf.data_ptr()) if Pbuf is not None else (None, None)

        normX2 = comm.allreduce_sum(gram(True))[0]
        phi_cache = {}
        # distance fields and support maps stay on the device when the geodesics run on this engine
        fields_on_device = getattr(compute_geodesic_distance, "_engine", None) is eng and hasattr(eng, "splocs_admm_fields")
        slot_of = {}
        if fields_on_device:
            eng.geodesic_cache_clear()
        trace, centres = [], []
        # the objective of every iteration stays on the device and is read once after the loop (nothing in the loop depends
        # on the printed numbers): with the distance fields on the device an outer iteration synchronises once, for its centres
        deferred = fields_on_device and hasattr(eng, "splocs_trace_begin") and num_iters_max > 0
        if deferred:
            eng.splocs_trace_begin(num_iters_max)
        for it in range(num_iters_max):
            cidx, cval = eng.splocs_weights(*ptrs())                          # :144-156, :161
            if comm.multi:
                cidx = comm.global_argmax(cidx, cval)
            if fields_on_device:
                wanted = [int(i) for i in dict.fromkeys(cidx.tolist())]
                missing = [i for i in wanted if i not in slot_of]
                if len(slot_of) + len(missing) > eng.GEODESIC_CACHE_SLOTS:    # cache full: start again with this iteration's centres
                    eng.geodesic_cache_clear()
                    slot_of, missing = {}, wanted
                if missing:
                    tol = getattr(compute_geodesic_distance, "_tol", 1e-13)
                    slot_of.update(zip(missing, eng.geodesic_cache_add(missing, tol)))
                eng.splocs_admm_fields([slot_of[int(i)] for i in cidx], lam, self.smooth_min_dist, self.smooth_max_dist,
                                       rho, num_admm_iterations)              # :162-181
            else:
                missing = [int(i) for i in dict.fromkeys(cidx.tolist()) if int(i) not in phi_cache]
                if missing:
                    many = getattr(compute_geodesic_distance, "solve_many", None)
                    phis = many(missing) if many else [compute_geodesic_distance(i) for i in missing]
                    for i, phi in zip(missing, phis):
                        phi_cache[i] = phi
                Lambda = np.empty((K, n_loc))
                for k in range(K):                                            # :162-165
                    phi = phi_cache[int(cidx[k])]
                    smap = (clip(phi, self.smooth_min_dist, self.smooth_max_dist) - self.smooth_min_dist) \
                        / (self.smooth_max_dist - self.smooth_min_dist)
                    Lambda[k] = lam * smap[v0:v0 + n_loc]
                eng.splocs_admm(Lambda, rho, num_admm_iterations)             # :167-181
            gram()
            centres.append(cidx.copy())
            if deferred:
                eng.splocs_objective_dev(it, *ptrs())
                continue
            wp, gm, sp = eng.splocs_objective(*ptrs())
            sparsity = comm.allreduce_sum(sp)[0]
            r2 = max(normX2 - 2.0 * wp + gm, 0.0)                             # |X - W C|^2
            E_rms = np.sqrt(r2) / sqrt(3 * N * F)
            energy = r2 + sparsity
            trace.append([energy, E_rms])
            if comm.rank == 0:
                print("itr %03d, Energy =%f, Error =%f" % (it, energy, E_rms))
        if deferred:
            tr = eng.splocs_trace(num_iters_max)                              # (its, 3): <W,P>, <G,M>, local sum Lambda |C_v|
            spars = comm.allreduce_sum(tr[:, 2].copy())
            for it in range(num_iters_max):
                r2 = max(normX2 - 2.0 * tr[it, 0] + tr[it, 1], 0.0)
                E_rms = np.sqrt(r2) / sqrt(3 * N * F)
                energy = r2 + spars[it]
                trace.append([energy, E_rms])
                if comm.rank == 0:
                    print("itr %03d, Energy =%f, Error =%f" % (it, energy, E_rms))
        C_loc, W_new = eng.splocs_results()
        self.splocs_comps = comm.all_gather_rows(C_loc, N, axis=1)
        self.splocs_weigs = W_new
        self.splocs_trace = np.array(trace)
        self.splocs_centres = np.array(centres, dtype=np.int64)

    @log_time("")
    def compute_components_store_singvalues(self):
        """posComponents.py:258-272."""
        headerSing = ['component', 'singVal', 'norm_R']
        self._comps_post_processed = False
        file_name = os.path.join(self.param.vertPos_output_directory,
                                 self.param.name + "_posBases_pcaExtraction_singValues_errorNorm")
        if self.storeSingVal:
            if self.pos_snapshots._comm.rank == 0:
                with open(file_name + '.csv', 'w', encoding='UTF8') as singFile:
                    writer = csv.writer(singFile)
                    writer.writerow(headerSing)
                    self.extract_k_components(writer)
            else:
                self.extract_k_components(None)
        else:
            self.extract_k_components(None)

    @log_time("")
    def post_process_components(self):
        """posComponents.py:274-302 on the device-resident basis: un-scale and add the mean
        (:279-282), per-dimension `orth` (:284-287: Gram -> K x K eigen-solve -> U = A V S^-1, the
        partial Gram matrices all-reduced over ranks), mass un-weighting (:289-292), then the
        reference's printed checks."""
        print("Post-processing pos components ...")
        snaps = self.pos_snapshots
        eng, comm = snaps._engine, snaps._comm
        v0, n_loc = snaps._shards[comm.rank]
        self._comps_streamed = False    # (the device basis is about to change: a later read copies it afresh)
        self._comps_post_processed = True       # (on_mesh_accuracy needs the basis in the tensor's space)
        if not self._comps_on_device:
            if self._comps is None:
                raise ValueError("no components: run compute_components_store_singvalues first")
            eng.components_upload(np.ascontiguousarray(self._comps[:, v0:v0 + n_loc, :]))      # caller-assigned comps
            self._comps_on_device = True
        later = bool(self.param.q_orthogonal or self.param.q_massWeight)       # (the basis is downloaded once, behind the last step)
        loc = eng.components_post(self.param.q_standarize, snaps.pre_scale_factor, None, download=not later)
        if self.param.q_orthogonal:
            K = self.numComp
            # Gram -> K x K Jacobi eigen-solver -> U = A V S^-1, all on the device (any K)
            Gbuf = comm.new_buffer(3 * K * K, eng.device_exchange) if comm.multi else None
            gp = Gbuf.data_ptr() if Gbuf is not None else None
            eng.orth_gram(gp)
            if Gbuf is not None:
                comm.allreduce_tensor(Gbuf)
            self.ortho_sing_vals = eng.orth_apply(gp)
            # the Gram route leaves U^T U = I + O(eps cond^2): one Newton-Schulz step with the Gram of U removes it
            Gbuf = comm.new_buffer(3 * K * K, eng.device_exchange) if comm.multi else None
            gp = Gbuf.data_ptr() if Gbuf is not None else None
            eng.orth_gram(gp)
            if Gbuf is not None:
                comm.allreduce_tensor(Gbuf)
            eng.orth_refine(gp)
            loc = None
        if self.param.q_massWeight:
            assert snaps.nVerts == snaps.invMassL.shape[0]
            loc = eng.components_post(False, 1.0, snaps.invMassL[v0:v0 + n_loc])
        if loc is None:
            loc = eng.results(want_comps=True, want_weigs=False)["comps"]
        self._comps = comm.all_gather_rows(loc, snaps.nVerts, axis=1)

        testSparsity(self.comps)
        test_linear_dependency(self.comps, 3, self.numComp)
        if self.param.q_orthogonal:
            self.is_utmu_orthogonal()
        print("... Volkwein (" + str(self.param.q_massWeight) + ")... standerized (" + str(self.param.q_standarize) +
              ")... support (" + str(self.support) + "), orthogonalized (" + str(self.param.q_orthogonal) + ").")

    @log_time("")
    def is_utmu_orthogonal(self):
        """posComponents.py:304-313."""
        print('... testing M orthogonality, U^T M U = I (K x K) ...', end='', flush=True)
        mass = self.pos_snapshots.mass
        if mass is None:        # (the reference needs q_massWeight here; without masses check U^T U = I)
            mass = np.ones(self.comps.shape[1])
        for l in range(self.comps.shape[2]):
            Mu_l = self.comps[:, :, l].T * mass[:, None]
            utMu_l = dot(self.comps[:, :, l], Mu_l)
            assert allclose(utMu_l, eye(self.comps.shape[0]))
        print('(True).')

    @log_time("")
    def store_components_to_files(self, start, end, step, fileType):
        """posComponents.py:315-327; fileType '.bin' or '.npy'."""
        print('Storing bases ...', end='', flush=True)
        numframes, numverts = self.pos_snapshots.frs, self.pos_snapshots.nVerts
        basesFile = os.path.join(self.param.vertPos_output_directory, self.fileNameBases)
        for k in range(start, end + 1, step):
            store_components(basesFile, numframes, k, numverts, 3, self.comps[:k, :, :], fileType, 'K')
        print('done.')

    @log_time("")
    def store_animations(self, output_bases_dir):
        """posComponents.py:329-341 (needs h5py, like the reference)."""
        import h5py
        output_components = os.path.join(output_bases_dir, self.output_components_file)
        with h5py.File(output_components, 'w') as f:
            f['default'] = self.pos_snapshots.verts[0]
            f['tris'] = self.pos_snapshots.tris
            for i, c in enumerate(self.comps):
                f['comp%03d' % i] = c

    @log_time("")
    def test_basesSingVals(self):
        """posComponents.py:343-356."""
        bases = self.comps.copy()
        s = empty((bases.shape[0], 3))
        for i in range(3):
            sing = svd(bases[:, :, i], full_matrices=False, compute_uv=False)
            s[:, i] = sing / sing.max()
        return s

    @log_time("")
    def test_convergence(self, start, end, step, writer=None):
        """posComponents.py:191-214 on the device: ``reconstruction_errors(start, end, step, "train")`` (one read of the
        prepared tensor in HBM; ``snapTensor`` is not downloaded and no (F, N, 3) reconstruction is formed)."""
        return self.reconstruction_errors(start, end, step, "train")

    # ------------------------------------------------------------------ extras: reconstruction errors, held-out projection
    def _device_basis(self):
        """The current basis in HBM (a basis assigned through the ``comps`` setter is uploaded first); returns K."""
        snaps = self.pos_snapshots
        eng, comm = snaps._engine, snaps._comm
        if not self._comps_on_device:
            if self._comps is None:
                raise ValueError("no components: run compute_components_store_singvalues first")
            C = np.asarray(self._comps, dtype=np.float64)
            if C.ndim != 3 or C.shape[1:] != (snaps.nVerts, 3):
                raise ValueError("components of shape %s do not match the %d vertices of the snapshots"
                                 % (C.shape, snaps.nVerts))
            v0, n_loc = snaps._shards[comm.rank]
            eng.components_upload(np.ascontiguousarray(C[:, v0:v0 + n_loc, :]))
            self._comps_on_device = True
            self._comps_streamed = False
        return eng.K

    def _heldout_prepare(self, verts):
        """Uploads a held-out (F', N, 3) animation, transforms it like the training tensor and factorises the Gram
        products of the current basis (sums over the ranks); returns the number of dependent components dropped."""
        snaps = self.pos_snapshots
        eng, comm = snaps._engine, snaps._comm
        if verts is None:
            raise ValueError("no test animation (pos_snapshots.test_verts is None)")
        Y = np.asarray(verts, dtype=np.float64)
        if Y.ndim != 3 or Y.shape[1:] != (snaps.nVerts, 3) or Y.shape[0] < 1:
            raise ValueError("held-out animation of shape %s: (F', %d, 3) expected" % (Y.shape, snaps.nVerts))
        self._device_basis()
        eng.heldout_upload(Y, snaps.massL, snaps._standarize, snaps.pre_scale_factor)
        Pbuf = Gbuf = None
        if comm.multi:
            Pbuf, Gbuf = comm.new_gram_buffers(Y.shape[0], eng.K, eng.device_exchange)
        eng.heldout_gram(Pbuf.data_ptr() if Pbuf is not None else None, Gbuf.data_ptr() if Gbuf is not None else None)
        if comm.multi:                 # partial Gram products: all-reduce (sum) over the ranks
            comm.allreduce_tensor(Pbuf)
            comm.allreduce_tensor(Gbuf)
        return eng.heldout_factor(Pbuf.data_ptr() if Pbuf is not None else None, Gbuf.data_ptr() if Gbuf is not None else None)

    def reconstruction_errors(self, start, end, step, animation="train"):
        """Extra (not in the reference): the error-against-k sweep of ``test_convergence`` (posComponents.py:192-249) for
        k in range(start, end + 1, step), as the same five lists ``fro_err, max_err, rel_err_x, rel_err_y, rel_err_z``.

        ``animation``: "train" -- the prepared training tensor with the greedy ``weigs`` and the current ``comps``, the
        reference's arithmetic; "test" -- ``pos_snapshots.test_verts``; or an (F', N, 3) ndarray.  A held-out animation is
        transformed like the training tensor (mass weighting, training mean row, training pre_scale_factor) and
        reconstructed with its least-squares weights on the first k components (the joint fit over all 3N coordinates).
        k = 0 gives the errors of the tensor itself.  Every rank returns the same lists."""
        snaps = self.pos_snapshots
        eng, comm = snaps._engine, snaps._comm
        if isinstance(animation, str) and animation not in ("train", "test"):
            raise ValueError("animation must be 'train', 'test' or an (F', N, 3) array, not %r" % animation)
        K = self._device_basis()
        if start < 0 or step < 1 or end > K:
            raise ValueError("range(%d, %d + 1, %d) is not a sweep over the %d components" % (start, end, step, K))
        train = isinstance(animation, str) and animation == "train"
        if train:
            if self.weigs is None or end > self.weigs.shape[1]:
                raise ValueError("no greedy weights for k = %d: run compute_components_store_singvalues first" % end)
        else:
            self._heldout_prepare(snaps.test_verts if isinstance(animation, str) else animation)
        ks = np.arange(start, end + 1, step, dtype=np.int64)
        S = ks.shape[0]
        if S == 0:
            return [], [], [], [], []
        sums, mx = np.empty((S, 3)), np.empty(S)
        norms = None
        for s0 in range(0, S, SWEEP_POINTS_PER_READ):
            s1 = min(S, s0 + SWEEP_POINTS_PER_READ)
            sums[s0:s1], mx[s0:s1], norms = eng.recon_sweep(0 if train else 1, ks[s0:s1])
        sums = comm.allreduce_sum(sums.reshape(-1)).reshape(S, 3)
        mx = comm.allreduce_max(mx)
        n2 = comm.allreduce_sum(norms[:3])
        tmax = comm.allreduce_max(norms[3:])[0]
        with errstate(divide='ignore', invalid='ignore'):
            fro_err = np.sqrt(sums.sum(axis=1))
            rel = np.sqrt(sums) / np.sqrt(n2)[None, :]
            max_err = mx / tmax
        return fro_err.tolist(), max_err.tolist(), rel[:, 0].tolist(), rel[:, 1].tolist(), rel[:, 2].tolist()

    def on_mesh_accuracy(self, r, frame_start=0, frame_end=None, frame_jump=1, animation="train", normals=True,
                         per_frame=False):
        """Extra (not in the reference's class): the on-mesh accuracy measures of ``compute_accuracy``
        (generate_figures/onMesh_accuracyMeasures.py:61-151) for the r-component reconstruction that
        ``reconstruction_errors`` uses for the same ``animation``, over the frames range(frame_start, frame_end, frame_jump),
        computed on the device in world space (mass weighting, mean row and scale undone).  With
        denom = sqrt(3 (frame_end - frame_start) N) (:70) the dict holds

        ``accum_norm`` (N,)      sum over the frames of frame_err[f, v] = |x - x_r|^2 / |x|^2 / denom (:116, :120)
        ``mesh_err`` (F_sel,)    |x - x_r|_F / |x|_F / denom of each frame (:117)
        ``accum_angle`` (N,)     with ``normals``: sum over the frames of the angle in degrees between the area-weighted
                                 per-vertex normals of the full and the reduced mesh (:73-90, :122-125)
        ``frame_err``, ``angle`` (F_sel, N), only with ``per_frame``
        ``stats`` (14,)          one CSV row without its first column, see ``store_on_mesh_measures``.

        A vertex in no triangle or with a zero normal has angle NaN, one with |x| = 0 an inf or NaN error, and the statistics
        carry them as NumPy's would.  Every rank returns the same dict; ``normals`` needs the triangles
        (``pos_snapshots.tris``) and one rank."""
        snaps = self.pos_snapshots
        eng, comm = snaps._engine, snaps._comm
        if isinstance(animation, str) and animation not in ("train", "test"):
            raise ValueError("animation must be 'train', 'test' or an (F', N, 3) array, not %r" % animation)
        if getattr(self, "_comps_post_processed", False):
            raise ValueError("the basis was un-scaled by post_process_components: the maps need it in the tensor's space "
                             "(call on_mesh_accuracy before post-processing, or recompute the components)")
        if normals and snaps.tris is None:
            raise ValueError("normals=True needs the mesh triangles (pos_snapshots.tris)")
        if normals and comm.multi:
            raise NotImplementedError("normals=True on several ranks: triangles straddle the vertex shards and no halo of "
                                      "reconstructed positions is built")
        K = self._device_basis()
        train = isinstance(animation, str) and animation == "train"
        if not 0 <= r <= K:
            raise ValueError("r = %d is outside 0..%d" % (r, K))
        if train:
            if self.weigs is None or r > self.weigs.shape[1]:
                raise ValueError("no greedy weights for r = %d: run compute_components_store_singvalues first" % r)
            F = snaps.frs
        else:
            Y = snaps.test_verts if isinstance(animation, str) else animation
            self._heldout_prepare(Y)
            F = np.asarray(Y).shape[0]
        frame_end = F if frame_end is None else frame_end
        if frame_jump < 1 or frame_start < 0 or frame_end > F or frame_start >= frame_end:
            raise ValueError("range(%d, %d, %d) is not a selection of the %d frames" % (frame_start, frame_end, frame_jump, F))
        N = snaps.nVerts
        n_sel = len(range(frame_start, frame_end, frame_jump))
        denom = float(np.sqrt(3 * (frame_end - frame_start) * N))
        if normals:
            eng.onmesh_mesh(snaps.tris)
        loc = eng.onmesh_run(0 if train else 1, r, frame_start, frame_end, frame_jump, normals, snaps.invMassL,
                             snaps._standarize, snaps.pre_scale_factor, denom, per_frame)
        out = {"accum_norm": comm.all_gather_rows(loc["accum_norm"], N, axis=0)}
        nd = comm.allreduce_sum(np.concatenate([loc["mesh_num"], loc["mesh_den"]]))
        with errstate(divide='ignore', invalid='ignore'):
            out["mesh_err"] = np.sqrt(nd[:n_sel]) / np.sqrt(nd[n_sel:]) / denom
        st = loc["stats"]
        sums = comm.allreduce_sum([st[1]])            # (angles: one rank)
        hi = comm.allreduce_max([-st[0], st[2], -st[3], st[4]])
        cnt = float(n_sel) * N
        stats = [-hi[2], sums[0] / cnt, hi[3], sums[0]]
        stats += [st[8], st[6] / cnt, st[9], st[6]] if normals else [np.nan] * 4
        stats += [-hi[0], sums[0] / N, hi[1]]
        stats += [st[5], st[6] / N, st[7]] if normals else [np.nan] * 3
        out["stats"] = np.array(stats, dtype=np.float64)
        if normals:
            out["accum_angle"] = loc["accum_angle"]
        if per_frame:
            out["frame_err"] = comm.all_gather_rows(loc["frame_err"], N, axis=1)
            if normals:
                out["angle"] = loc["angle"]
        return out

    def store_on_mesh_measures(self, r_values, output_dir, case="_test_on_training_set", **range_args):
        """Extra: writes ``_on_mesh_measures<case>.csv`` with the header of onMesh_accuracyMeasures.py:95-98 and one row per r,
        composed as its commented-out writer does (:132-137): r; min / mean / max / sum of frame_err; the same of angle;
        min / mean / max of accum_norm; min / mean / max of accum_angle.  ``range_args`` go to ``on_mesh_accuracy``.  The
        statistics come from the device pass: the (F_sel, N) maps are not downloaded.  Returns the rows."""
        rows = [[int(r)] + self.on_mesh_accuracy(r, **range_args)["stats"].tolist() for r in r_values]
        if self.pos_snapshots._comm.rank == 0:
            with open(os.path.join(output_dir, "_on_mesh_measures" + case) + '.csv', 'w', encoding='UTF8') as acc_file:
                writer = csv.writer(acc_file)
                writer.writerow(_u.ON_MESH_HEADER)
                writer.writerows(rows)
        return rows

    def project_animation(self, verts=None):
        """Extra (not in the reference): the (F', K) least-squares weights of an (F', N, 3) animation (None: the test
        animation, ``pos_snapshots.test_verts``) on the current basis, in the standardised, mass-weighted space of the
        training tensor: W = P G^-1 with P = Y C^T, G = C C^T.  A component that depends on the earlier ones gets weight 0."""
        snaps = self.pos_snapshots
        self._heldout_prepare(snaps.test_verts if verts is None else verts)
        return snaps._engine.heldout_weights()

    @staticmethod
    def frobenius_error(f, f_reconstructed):
        """posComponents.py:217-223."""
        return norm(f - f_reconstructed)

    @staticmethod
    def relative_error_per_component(f, f_reconstructed):
        """posComponents.py:225-237."""
        return [norm(f[:, :, i] - f_reconstructed[:, :, i]) / norm(f[:, :, i]) for i in range(3)]

    @staticmethod
    def max_pointwise_error(f, f_reconstructed):
        """posComponents.py:239-249."""
        return np.max(np.abs(f - f_reconstructed)) / np.max(f)
