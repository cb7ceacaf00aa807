/*
 * asb.h -- C ABI of libasb_hip.so: the MI355X (gfx950) implementation of the
 * animSnapBases snapshot-reduction hot path.
 *
 * The reference (ShMonem/animSnapBases) is pure Python and has NO FFI / plugin
 * interface for this path: the drop-in boundary is the Python class
 * API (posSnapshots / posComponents), mirrored in animsnapbases_amd/.  This header is
 * the thin C ABI underneath it; every entry point names the reference lines whose
 * arithmetic it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - plain C: pointers, int64_t sizes, doubles.  No torch / numpy types.
 *   - return 0 on success, a negative asb_status otherwise; text via asb_last_error().
 *   - host buffers are caller-owned, C-contiguous, float64 / int64.
 *   - pointers named *_dev are DEVICE pointers owned by the caller (e.g. the storage of
 *     a torch tensor used for an RCCL collective); all other device memory belongs to
 *     the context.
 *   - a context is bound to one GPU and one HIP stream and is not thread-safe.
 *   - all work is enqueued on the context's stream; calls that return host data
 *     synchronise that stream, all others are asynchronous.
 *
 * Device layout ("vertex-major"): the (F, N, 3) snapshot tensor of the reference is held
 * as rows r = 3*v + d of Fp = roundup(F, 16) doubles, row r at byte offset r*Fp*8, so that
 * a vertex's 3 x F trajectory is one contiguous 24*Fp-byte run.  Padding entries are 0.
 * Multi-GPU: each context owns the contiguous vertex range [v0, v0 + n_loc).
 */
#ifndef ASB_H
#define ASB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASB_ABI_VERSION 1

typedef struct asb_ctx asb_ctx;

typedef enum asb_status {
    ASB_OK = 0,
    ASB_ERR_ARG = -1,      /* bad argument / wrong call order            */
    ASB_ERR_HIP = -2,      /* HIP runtime error (text has the HIP string) */
    ASB_ERR_NODEV = -3,    /* no usable gfx950 device                     */
    ASB_ERR_LIMIT = -4,    /* size outside what the kernels are built for */
    ASB_ERR_NUMERIC = -5   /* numerical breakdown (e.g. Cholesky pivot)   */
} asb_status;

/* ---------------------------------------------------------------- context ---- */
int asb_abi_version(void);
/* stream: a hipStream_t to enqueue on (e.g. torch's current stream so that RCCL
 * collectives issued by torch.distributed are ordered with the kernels), NULL for a
 * private stream, or ASB_STREAM_DEFAULT for the device's default (null) stream -- which is
 * what torch's current stream is unless the caller switched streams. */
#define ASB_STREAM_DEFAULT ((void*)(intptr_t)-1)
int asb_create(int device_id, void* hip_stream, asb_ctx** out);
void asb_destroy(asb_ctx* ctx);
const char* asb_last_error(const asb_ctx* ctx);
int asb_sync(asb_ctx* ctx);
/* number of launches of the dominant streaming kernel and their total HIP-event time
 * (ms) since the last reset; used by bench.py for the roofline figure. */
int asb_prof_reset(asb_ctx* ctx, int enable);
int asb_prof_get(asb_ctx* ctx, int64_t* launches, double* total_ms);

/* ------------------------------------------------- snapshot preparation ------ */
/* posSnapshots.do_snapshots_precomputations, snapbases/posSnapshots.py:64-105.
 * X: host (F, N_glob, 3).  Uploads vertices [v0, v0+n_loc), multiplies row v by
 * massL[v0+v] when massL != NULL (:82) and stores the vertex-major layout. */
int asb_snapshots_upload(asb_ctx* ctx, const double* X, int64_t F, int64_t N_glob,
                         int64_t v0, int64_t n_loc, const double* massL);
/* Same, but X_dev is already in device memory in the reference layout (F, n_loc, 3)
 * (synthetic benchmark inputs generated on the GPU): this rank's vertices [v0, v0+n_loc)
 * of N_glob. */
int asb_snapshots_adopt_dev(asb_ctx* ctx, const double* X_dev, int64_t F, int64_t n_loc,
                            const double* massL_loc, int64_t v0, int64_t N_glob);
/* :85-89 + posSnapshots.standarize :168 -- mean = frame 0 (rest_shape 0) or the frame
 * average (1); when subtract != 0 the mean row is subtracted.  local_sum = sum of all
 * entries of the shard afterwards (for the global mean of np.std). */
int asb_snapshots_center(asb_ctx* ctx, int rest_shape, int subtract, double* local_sum);
/* asb_snapshots_upload / asb_snapshots_adopt_dev followed by asb_snapshots_center in ONE sweep over the data: with
 * rest_shape 0 ("first", :86) the rest row is frame 0 of the input, so the layout change subtracts it on the fly and also
 * returns sums_out[0] = sum(x) and sums_out[1] = sum(x^2) of the prepared shard (np.std of :170 then needs no sweep of its
 * own: var = sum(x^2)/n - mu^2, the caller falls back to asb_snapshots_sqdev when mu^2 >> var).  rest_shape 1 ("average")
 * runs the separate sweeps and returns sums_out[1] = -1. */
int asb_snapshots_upload_rest(asb_ctx* ctx, const double* X, int64_t F, int64_t N_glob, int64_t v0, int64_t n_loc,
                              const double* massL, int rest_shape, int subtract, double* sums_out);
int asb_snapshots_adopt_dev_rest(asb_ctx* ctx, const double* X_dev, int64_t F, int64_t n_loc, const double* massL_loc,
                                 int64_t v0, int64_t N_glob, int rest_shape, int subtract, double* sums_out);
/* sum over the shard of (x - mu)^2 -- second pass of np.std, :171 */
int asb_snapshots_sqdev(asb_ctx* ctx, double mu, double* local_sqdev);
/* snapTensor *= pre_scale_factor, :172 */
int asb_snapshots_scale(asb_ctx* ctx, double pre_scale_factor);
int asb_snapshots_get_mean(asb_ctx* ctx, double* mean_out /* (n_loc,3) */);
/* the prepared tensor back in the reference layout, out: (F, n_loc, 3) */
int asb_snapshots_download(asb_ctx* ctx, double* out);

/* ------------------------------------- greedy deflation ("PCA") -------------- */
/* posComponents.extract_k_components, snapbases/posComponents.py:67-122.
 *
 * mode ASB_DEFLATE_RESIDUAL keeps the residual tensor R in HBM and updates it per
 * component exactly as the reference does (needed for support='local').
 * mode ASB_DEFLATE_PROJECT is the residual-free form valid for support='global':
 * the weights w_k are mutually orthogonal there, so c_k = X^T w_k / |w_k|^2 and X is
 * only ever READ. */
#define ASB_DEFLATE_RESIDUAL 0
#define ASB_DEFLATE_PROJECT 1
int asb_deflate_begin(asb_ctx* ctx, int64_t K, int mode, int local_support);
/* number of doubles of one exchange record: [energy, idx (int64 bits), slab 3*Fp] */
int64_t asb_deflate_xchg_len(const asb_ctx* ctx);
/* :78-80 on this shard: best local vertex (max residual energy, first on ties) and
 * its 3 x F residual slab -> rec_dev (one record). */
int asb_deflate_local_best(asb_ctx* ctx, int64_t k, double* rec_dev);
/* :79-96: winner over n_rec records (max energy, lowest global index), rank-1 SVD of
 * its 3 x F slab, w_k = sigma_1 * Vt[0]; with local_support also the +-projection
 * test :90-94.  recs_dev == NULL: single rank, reads the shard directly. */
int asb_deflate_pick(asb_ctx* ctx, int64_t k, const double* recs_dev, int64_t n_rec);
/* selected vertex (global index) and sigma_1 of component k (synchronises) */
int asb_deflate_get_pick(asb_ctx* ctx, int64_t k, int64_t* idx, double* sigma);
/* 'pca_blocks' constraint bases (snapbases/constraintsComponents.py:324-412; residual mode).
 * asb_deflate_block_argmax: the constraint (block of p consecutive rows) with the largest residual energy on this
 * shard -- indxLargestDeformation, :86-92 (first maximum); the shard must hold whole blocks; block_out is global.
 * asb_deflate_force_next: the next asb_deflate_local_best / asb_deflate_pick takes global row gidx instead of the
 * arg-max (the reference deflates the p rows of the chosen constraint one after the other, :352-356). */
int asb_deflate_block_argmax(asb_ctx* ctx, int p, int64_t* block_out, double* val_out);
int asb_deflate_force_next(asb_ctx* ctx, int64_t gidx);
/* :101-111: c_k = (w_k . R)[* s] / |w_k|^2, R -= w_k (x) c_k, new energies.
 * s: host (n_loc) support factor 1 - support_map (:95), or NULL for global. */
int asb_deflate_apply(asb_ctx* ctx, int64_t k, const double* s);
/* components k0 .. k1-1 back to back on one rank with global support (no host round
 * trips inside). */
int asb_deflate_run_global(asb_ctx* ctx, int64_t k0, int64_t k1);
/* outputs.  comps (K, n_loc, 3); weigs (F, K); idx (K) global indices; sigma (K);
 * normR2_local (K): this shard's ||R||_F^2 after each component (:113, summed over
 * shards and square-rooted by the caller). Any pointer may be NULL. */
int asb_deflate_results(asb_ctx* ctx, double* comps, double* weigs, int64_t* idx,
                        double* sigma, double* normR2_local);
/* ---- projection mode, panel by panel (what asb_deflate_run_global does internally on one
 * rank; the multi-rank driver interleaves the collectives marked [ALL-*]) ------------------
 *   asb_panel_scale                     [ALL-REDUCE max of e0max, then set it on every rank]
 *   per panel:
 *     asb_panel_hist/tau(1), (2)  (local)  asb_panel_top_energies  [ALL-GATHER cap+1 doubles]  asb_panel_global_tau
 *     asb_panel_select(rows, ids behind the rows)  [ALL-GATHER rows+ids]  asb_panel_assemble_packed
 *     asb_panel_run(_spec) -> steps (identical on every rank: same data, same arithmetic)
 *     asb_panel_project    (local shard)   | with unproven steps: asb_panel_project_spec [ALL-REDUCE min] asb_panel_commit
 *   (older form, still supported: histograms all-reduced per level, rows and ids gathered separately)           */
int asb_panel_scale(asb_ctx* ctx, double* normX2_local, double* e0max_local, double set_e0max);
/* local energy histogram (ASB_NBINS = 2048 ints) into hist_dev (NULL: internal) */
int asb_panel_hist(asb_ctx* ctx, int level, int* hist_dev);
/* threshold step from the (summed) histogram; the histogram is consumed (cleared to zero) */
int asb_panel_tau(asb_ctx* ctx, int level, const int* hist_dev);
/* One-exchange thresholding for several ranks: after the LOCAL histogram steps (hist_dev = NULL, no all-reduce),
 * asb_panel_top_energies writes this shard's energies above its local threshold into out_dev[0 .. cap) (unordered,
 * padded with -1) and that local threshold into out_dev[cap].  The ranks all-gather the cap + 1 doubles; the global
 * threshold tau = max((m_target + 1)-th largest exported energy, max of the local thresholds) is installed with
 * asb_panel_set_tau (device scalar) on every rank.  asb_panel_target: m_target. */
int asb_panel_top_energies(asb_ctx* ctx, double* out_dev, int64_t cap);
/* the same selection on the device: tab_dev = the all-gathered (world, cap + 1) exports; installs tau and returns the
 * per-rank candidate counts (host, world).  ASB_ERR_LIMIT when world * cap does not fit the selection kernel's LDS. */
int asb_panel_global_tau(asb_ctx* ctx, const double* tab_dev, int world, int64_t cap, int64_t* counts_out);
int asb_panel_set_tau(asb_ctx* ctx, const double* tau_dev);
int64_t asb_panel_target(const asb_ctx* ctx);
/* this shard's candidates (energy > tau; every vertex when global_all; only forced_gidx when
 * >= 0), in vertex order, and their exact residual rows (3*Fp doubles each) into the caller's
 * device buffers of capacity asb_panel_capacity() (NULL: the context's own buffer).
 * n_local / overflow (optional) synchronise. */
int asb_panel_select(asb_ctx* ctx, int64_t k, int64_t forced_gidx, int global_all, double* rows_out_dev,
                     long long* idx_out_dev, int64_t* n_local, int* overflow);
int64_t asb_panel_capacity(const asb_ctx* ctx);
/* 1 if the co-resident panel kernel can run on this context (switched on, and F <= 2048 so that a candidate row fits its
 * registers), else 0.  Several sub-panels per read and asb_panel_read_run need it; a driver asks before taking them. */
int asb_panel_coop_possible(const asb_ctx* ctx);
/* replicated candidate buffer from the all-gathered padded pieces:
 * rows_g_dev (world, maxcount, 3, Fp), idx_g_dev (world, maxcount), counts (host, world) */
int asb_panel_assemble(asb_ctx* ctx, const double* rows_g_dev, const long long* idx_g_dev,
                       const int64_t* counts, int world, int64_t maxcount);
/* the same from ONE all-gathered buffer (one collective instead of two): every rank's piece is its maxcount rows
 * followed by its maxcount vertex ids (int64), maxcount * (3*Fp + 1) eight-byte words per rank -- i.e. asb_panel_select
 * was given idx_out_dev = (long long*)(rows_out_dev + maxcount * 3*Fp) */
int asb_panel_assemble_packed(asb_ctx* ctx, const double* packed_g_dev, const int64_t* counts, int world, int64_t maxcount);
/* up to `steps` (<= 16) greedy steps on the candidate buffer; *committed of them are final */
int asb_panel_run(asb_ctx* ctx, int64_t k0, int steps, int global_all, int assembled, int64_t* committed);
/* one pass over X for components [k0, k0+ncols): c_k on this shard, energies */
int asb_panel_project(asb_ctx* ctx, int64_t k0, int ncols);
/* Multi-rank form of the unproven steps (asb_deflate_spec_stats): asb_panel_run_spec lets the panel kernel append up to
 * spec_max steps whose winner is not provable in advance (*ran steps in all, the first *proven of them certain; identical
 * on every rank).  asb_panel_project_spec is the pass over X for all of them with the energies left untouched;
 * *first_rejected = first unproven step that one of THIS shard's vertices contradicts (ncols: none).  The caller takes
 * the minimum over the ranks and asb_panel_commit applies the energies of that many columns (0: nothing stood).
 * asb_panel_commit belongs to the asb_panel_project_spec[_dev] before it: it commits that pass and counts the kept unproven
 * steps against that call's `proven`; it must not follow any other pass. */
int asb_panel_run_spec(asb_ctx* ctx, int64_t k0, int steps, int global_all, int assembled, int spec_max, int64_t* ran,
                       int64_t* proven);
int asb_panel_project_spec(asb_ctx* ctx, int64_t k0, int ncols, int proven, int64_t* first_rejected);
int asb_panel_commit(asb_ctx* ctx, int64_t k0, int kept);
/* asb_panel_project_spec without the host read-back: the count is written (as a float64) to the caller's device word,
 * which the multi-rank driver min-all-reduces and reads once (one host synchronisation per panel instead of two). */
int asb_panel_project_spec_dev(asb_ctx* ctx, int64_t k0, int ncols, int proven, double* first_rejected_dev);
/* fallback: exact energies of every vertex of the shard; optional first arg-max */
int asb_panel_refresh(asb_ctx* ctx, int64_t k, double* best_energy, int64_t* best_gidx);

/* projection mode statistics of the last run: streaming passes over X (panels) and exact
 * energy refreshes (fallback when the energy recurrence could not prove a candidate). */
int asb_deflate_stats(asb_ctx* ctx, int64_t* n_panels, int64_t* n_refresh);
/* panels may append steps whose winner could not be proven in advance (bound on the vertices outside the candidate set
 * too stale); the projection pass then checks them against every vertex's energy and keeps the valid prefix, so the
 * selected sequence stays that of the reference loop (posComponents.py:75-77).  tried / kept: such steps in the last
 * run.  ASB_SPEC_PANELS=0 switches them off. */
int asb_deflate_spec_stats(asb_ctx* ctx, int64_t* tried, int64_t* kept);
/* reads of the snapshot tensor that the last asb_deflate_begin spent on the initial per-vertex energies ((R**2).sum of
 * posComponents.py:78-80 at k = 0): 0 when they came with the standardisation sweep (asb_snapshots_scale) or with an
 * earlier begin on the same, unchanged tensor; 1 otherwise.  ASB_E0_REUSE=0 always recomputes them. */
int asb_deflate_energy_passes(asb_ctx* ctx, int64_t* n_passes);
/* The panel's inner loop normally runs as ONE launch of co-resident blocks that exchange records through memory
 * (k_panel_coop).  If that exchange times out -- the blocks were not all resident because something else shares the GPU --
 * the panel is redone by the two-kernel loop and the context stays on it; *n = how often that happened (lifetime). */
int asb_deflate_coop_fallbacks(asb_ctx* ctx, int64_t* n);
/* First panel of a tensor whose energy sits largely (> 1/4) in the constant-in-time direction (rest shape "first" on
 * noise-like data): its candidates are guessed from the energies without that direction (a by-product of
 * asb_snapshots_scale) in addition to the few largest initial energies; the steps taken on the guess are unproven steps
 * like any others (asb_deflate_spec_stats), so the sequence is still that of posComponents.py:75-77.  *n = 1 if the last
 * run did so.  ASB_FIRST_PANEL_MEAN=0 switches it off. */
int asb_deflate_guessed_panels(asb_ctx* ctx, int64_t* n);
/* Of the last run: launches of the co-resident panel kernel (0 when F > 2048: every panel took the two-kernel loop), and
 * the most components one read of X committed over all its sub-panels (above 64: more than four tiles in one read). */
int asb_deflate_read_stats(asb_ctx* ctx, int64_t* coop_launches, int64_t* max_read_kept);
/* Structured data (every component removes a direction all vertices share): the energies at the start of a read no longer
 * say who wins a few steps later, and its pass rejects most of its unproven steps.  The coefficient columns of those rejected
 * steps are a rank-r sketch of every vertex's residual; a greedy replay of posComponents.py:76-96 in that space (asb_sketch.hip:
 * one thread per vertex, the sketch in registers) names the NEXT read's candidates.  Only the candidates change: every step is
 * still checked by the pass against every vertex outside them, so the selected sequence stays the reference's.
 * A replay runs only if the sketch holds at least 0.15 of the residual's energy -- on noise it holds r / F of it and
 * candidates by energy do as well; the kernel decides that itself (one exchange) and otherwise leaves the plain selection.
 * *runs = replays in the last run, *reads = reads of X whose candidates came from one.  ASB_SKETCH=0 switches it off. */
int asb_deflate_sketch_stats(asb_ctx* ctx, int64_t* runs, int64_t* reads);
/* Leaving the projection mode in mid-run.  The panel algorithm proves its winners against bounds kept in the energy recurrence;
 * where that cannot work -- K beyond the numerical rank of the data: the residual is rounding noise, nothing is provable and
 * every panel ends in an exact refresh, ~5 reads of X per component -- the reference's own loop (posComponents.py:76-96: keep R,
 * one read + one write per component) is the cheaper algorithm.  asb_project_switch_residual(ctx, k), k = components committed
 * so far: R_k = X - sum_{j<k} w_j (x) c_j is written out once, the per-component scalars are converted, and the context is in
 * residual mode from there on (asb_deflate_local_best / _pick / _apply / _results as if the run had begun in it).
 * asb_deflate_run_global does this by itself (single rank) once the reads of X of the last >= 8 committed fewer than 3/4 of a
 * component each (ASB_STALL_FALLBACK=0: never); several ranks: the driver applies the same rule (_panels.py).
 * asb_deflate_switch_stats: the component at which the last run switched, -1 if it did not. */
int asb_project_switch_residual(asb_ctx* ctx, int64_t k);
/* The multi-rank read of X in two calls and ONE exchange (round 4; what asb_deflate_run_global does inside the library on one
 * rank: posComponents.py:76-96 for up to 64 components per read).  Every rank holds the same assembled candidates
 * (asb_panel_assemble*).  asb_panel_read_run: all (<= nsub_max) sub-panels of the read in ONE launch of the panel kernel --
 * identical on every rank --, this shard's pass over X and the checks of all tiles behind it; words_dev (device, 10 doubles):
 * [ct] = columns of tile ct that stand on this shard (the tile's length if it was not reached: neutral under min), [8] = status
 * (0; -1: the kernel's exchange timed out here), [9] = the local counts again, packed, NOT to be reduced.  The driver
 * min-all-reduces words_dev[0 .. 8] over the ranks, reads all 10 words once (asb_fetch_doubles) and hands them to
 * asb_panel_read_commit: tiles stand in full while the minimum equals their length, the first one below keeps that many
 * columns, nothing behind it; a shard whose local chain ran ahead of the verdict rolls its energies back first.  With status
 * -1 the driver passes zeros (roll-back only), switches the kernel off on all ranks (asb_panel_set_coop) and repeats the panel. */
/* SPLOCS without a host read per outer iteration (posComponents.py:183-189 prints one line per iteration; nothing in the loop
 * depends on the printed numbers): asb_splocs_trace_begin sizes a device trace and defers the ADMM's status check,
 * asb_splocs_objective_dev leaves iteration it's <W,P>, <G,M>, sum Lambda |C_v| there, asb_splocs_trace reads all (n_its, 3) once. */
int asb_splocs_trace_begin(asb_ctx* ctx, int64_t n_its);
int asb_splocs_objective_dev(asb_ctx* ctx, const double* P_dev, const double* M_dev, int64_t it);
int asb_splocs_trace(asb_ctx* ctx, int64_t n_its, double* out_n_its_by_3);
int asb_panel_read_run(asb_ctx* ctx, int64_t k0, int64_t k1, int nsub_max, int spec_budget, const int* sub_budget8,
                       double* words_dev, int* ntile_out, int* nc_out8, int* proven_out8);
int asb_panel_read_commit(asb_ctx* ctx, const double* words10_host, int64_t* total_out, int* full_out, int* rejected_out);
int asb_fetch_doubles(asb_ctx* ctx, const double* dev, int n, double* out);
int asb_deflate_switch_stats(asb_ctx* ctx, int64_t* k_switch);
/* The same for the multi-rank driver (animsnapbases_amd/_panels.py).  asb_panel_guess_stats: this shard's energy along the
 * constant direction, its |X|^2 and whether the context could guess at all (0: both values are 0); the ranks sum all three
 * and guess only if every rank can and the share exceeds 1/4.  asb_panel_guess_begin (before the first panel's
 * asb_panel_hist): installs the score thresholds (each rank its share 1/world of the targets) and a smaller target for the
 * energies proper, which asb_panel_tau / asb_panel_global_tau / asb_panel_target then use; asb_panel_select takes the
 * union (the counts returned by asb_panel_global_tau do not include it: ask asb_panel_select for them);
 * asb_panel_project_spec* check against the same union.  asb_panel_guess_end (after that panel, whatever its outcome)
 * restores the plain selection. */
int asb_panel_guess_stats(asb_ctx* ctx, double* mean_energy_local, double* normx2_local, int* possible);
int asb_panel_guess_begin(asb_ctx* ctx, int world);
int asb_panel_guess_end(asb_ctx* ctx);
/* Multi-rank runs (assembled candidate buffer): a timed-out exchange is NOT redone locally -- the ranks must stay in
 * lock-step -- asb_panel_run / asb_panel_run_spec then return *committed = -1 with the kernel switched off for this context;
 * the driver min-reduces that over the ranks, switches it off everywhere (asb_panel_set_coop, returns the old setting) and
 * repeats the panel on every rank. */
int asb_panel_set_coop(asb_ctx* ctx, int on);
/* *out = *dev (one float64 in device memory, e.g. the min-all-reduced count of asb_panel_project_spec_dev) in stream order,
 * published into pinned host memory and polled there instead of a stream synchronisation */
int asb_fetch_double(asb_ctx* ctx, const double* dev, double* out);
/* the final residual in the reference layout (F, n_loc, 3) (R of :125) */
int asb_deflate_download_residual(asb_ctx* ctx, double* out);

/* ------------------------------------------------ post-processing ------------ */
/* posComponents.post_process_components, snapbases/posComponents.py:277-292, the
 * element-wise part, in place on the device-resident components:
 *   unscale != 0:  comps /= pre_scale_factor; comps += mean        (:279-282)
 *   invMassL != NULL (host, n_loc entries of this shard): comps *= invMassL[:,None] (:292)
 * comps_out (K, n_loc, 3) may be NULL. */
int asb_components_post(asb_ctx* ctx, int unscale, double pre_scale_factor,
                        const double* invMassL_loc, double* comps_out);

/* :284-287 `comps[:,:,l] = orth(comps[:,:,l].T).T` (scipy's SVD-based orth) per dimension,
 * as Gram (MFMA) -> K x K Jacobi eigen-solve -> U = A V S^-1, all on the device (K <= 128: parallel Jacobi in one
 * block's LDS; larger K: one-sided Jacobi on the rows of the Gram matrix, csrc/asb_smalldense.hip).
 * asb_orth_gram: this shard's three K x K Gram matrices into G_dev (3*K*K doubles, caller's
 * device buffer to be all-reduced over ranks) or into the context when NULL.
 * asb_orth_apply: finishes with the (summed) Gram matrices; sing_out (host, 3*K, optional).
 * Fails with ASB_ERR_NUMERIC when a slice is rank deficient (orth would drop vectors).
 * asb_orth_refine: second pass -- with the Gram matrices of the basis asb_orth_apply left (asb_orth_gram again,
 * summed), one symmetric Newton-Schulz step U <- U (1.5 I - 0.5 U^T U): squares the eps * cond^2 orthogonality
 * defect of the Gram route, so U^T U = I holds to round-off like scipy's SVD-based orth. */
int asb_orth_gram(asb_ctx* ctx, double* G_dev);
int asb_orth_apply(asb_ctx* ctx, const double* G_dev, double* sing_out);
int asb_orth_refine(asb_ctx* ctx, const double* G_dev);
/* K > 128 (the one-block eigen-solver / Cholesky of asb_orth_apply / asb_qr_apply stop there): the K x K step of
 * the orthogonalisation runs on the host.  asb_orth_gram_get: the three Gram matrices of asb_orth_gram (NULL buffer)
 * to the host; asb_components_transform: comps[:, :, l] <- sum_i comps_i T[l][i][j] with T host (3, K, K) --
 * T_l = V S^-1 (orth, :284-287) or L^-T (qr, constraintsComponents.py:431-435). */
int asb_orth_gram_get(asb_ctx* ctx, double* G_host);
int asb_components_transform(asb_ctx* ctx, const double* T_host);
/* geom_constructed, constraintsComponents.py:489-521, the large product: out (host, F x n_loc x 3),
 * out[f][e][l] = sum_{j < r} comps[j][e][l] coef[l][j][f] with coef host (3, r, F) (the interpolation coefficients of
 * every frame, solved by the caller from the r p x r p normal equations as the reference does) */
int asb_components_expand(asb_ctx* ctx, const double* coef_host, int64_t r, int64_t F, double* out_host);
/* the device-resident basis (K, n_loc, 3) to the host */
int asb_components_download(asb_ctx* ctx, double* comps_out);
/* ---- the weighted differential operator S^T of the constraint path (constraintsComponents.py:70-74: a scipy sparse matrix
 * read from an .npz; rows = position-space vertices, columns = the e p constraint rows).  asb_st_upload and the two calls
 * below need all constraint rows on this rank; several ranks use the asb_st_*shard* calls further down. */
int asb_st_upload(asb_ctx* ctx, int64_t n_rows, int64_t n_cols, int64_t nnz, const int64_t* indptr_host,
                  const int64_t* indices_host, const double* data_host);
/* 'pca_blocks_with_St' (constraintsComponents.py:180): v = argmax_rows sum((S^T R_flat)^2) on the CURRENT residual of the
 * residual-mode deflation (R_flat = (e p) x (3 F)); first maximum */
int asb_st_residual_argmax(asb_ctx* ctx, int64_t* v_out, double* val_out);
/* |R|_F^2 of the residual-mode deflation right now (the loop condition `while norm(R) > tol`, :179, :252) */
int asb_deflate_residual_norm2(asb_ctx* ctx, double* out);
/* residual mode: room for K_new >= K components in all; W / comps / scalars grow, what the run produced so far is kept (loops
 * that end on a tolerance -- :179 `while norm(R) > tol` -- reserve a little and grow geometrically, as the reference's lists do) */
int asb_deflate_reserve(asb_ctx* ctx, int64_t K_new);
/* geom_block_form_utilizing_differential_operator(error_in_pos_space=True) (:652-672): residual of basis block k as
 * asb_deim_block_residual, mapped to position space by S^T ((|V|) x (3 p)); first arg-max of its squared row norms */
int asb_deim_block_residual_st(asb_ctx* ctx, int64_t k, int p, const double* coef_host, double* maxabs_out, int64_t* v_out,
                               double* val_out);
/* ---- S^T with the constraint rows sharded over several ranks.  A position vertex belongs to the rank holding the smallest
 * column of its S^T row (rank 0 for an empty row); the HALO are the h constraint rows its owned vertices reference on other
 * ranks, kept here as copies.  The caller computes ownership and halo on the host and uploads the owned rows' CSR with the
 * columns remapped to local slots: [0, n_loc) rows of this shard, [n_loc, n_loc + h) halo slots (sorted halo rows), each
 * row in the global row's column order (every sum then runs in the one-rank order).  Valid until the next upload. */
int asb_st_upload_shard(asb_ctx* ctx, int64_t n_own, int64_t nnz, const int64_t* indptr_host, const int64_t* slots_host,
                        const double* data_host, int64_t n_halo);
/* The exchange that fills the halo, which 0: rows of the residual-mode residual (after asb_deflate_begin; 3 Fp doubles per
 * row), which 1: rows of the device basis (3 K doubles per row, [j][i]).  pack: the rows gidx (global, on this shard) into
 * out_dev (device, n x row length); fill: halo slot s <- row slot_host[s] < n_src of src_dev (device, the rows of every rank
 * gathered, n_src x row length).  Synchronises the context's stream. */
int asb_st_halo_pack(asb_ctx* ctx, int which, const int64_t* gidx_host, int64_t n, double* out_dev);
int asb_st_halo_fill(asb_ctx* ctx, int which, const double* src_dev, const int64_t* slot_host, int64_t n_src);
/* after asb_deflate_apply(k): the same deflation of the halo residual (same k_stream pass, same w_k), so every halo row
 * stays equal to its owner's row bit for bit; its energies do not count towards |R|^2 */
int asb_st_halo_deflate(asb_ctx* ctx, int64_t k);
/* asb_st_residual_argmax over the OWNED vertices: first arg-max as an index into them (-1 when there are none) */
int asb_st_shard_residual_argmax(asb_ctx* ctx, int64_t* v_loc_out, double* val_out);
/* asb_deim_block_residual_st over the owned vertices (halo basis rows: asb_st_halo_fill 1 for the current basis); the
 * caller max-reduces *maxabs_out and takes the global arg-max */
int asb_deim_block_residual_st_shard(asb_ctx* ctx, int64_t k, int p, const double* coef_host, double* maxabs_out,
                                     int64_t* v_loc_out, double* val_out);
/* out4 = [halo rows h, owned vertices, their S^T entries, K of the halo basis (0: none)] */
int asb_st_shard_stats(asb_ctx* ctx, int64_t* out4);
/* the halo copies to the host: which 0 (h, 3, F) residual rows, 1 (K, h, 3) basis rows */
int asb_st_halo_download(asb_ctx* ctx, int which, double* out_host);
/* The basis into PINNED host memory, overlapped with the run that produces it (posComponents.py:119 leaves `comps` in host
 * memory: `self.comps = array(C)`).  asb_components_stream(ctx, 1) before asb_deflate_begin: the context keeps a pinned
 * (K, n_loc, 3) buffer and a copy stream; every component row is copied as soon as it is final (projection mode: after each
 * read of X, while the next read runs; otherwise at the end).  asb_components_pinned waits for the copies and returns the
 * buffer: valid until the next asb_deflate_begin / destroy on this context (the caller copies what it wants to keep).
 * asb_components_stream(ctx, 0) switches it off and frees the buffer.
 * asb_components_stream_into: the same into a pinned buffer the CALLER owns (`count` doubles >= K n_loc 3 of the runs that
 * follow, or asb_deflate_begin fails; NULL: off) -- for callers that hand the buffer on (the Python engine's ndarray views):
 * the context never frees it and stops writing to it with the next _into / asb_components_stream(ctx, 0) / asb_destroy.
 * asb_host_alloc / asb_host_free: pinned host memory for such a buffer (hipHostMalloc / hipHostFree; no context). */
int asb_components_stream(asb_ctx* ctx, int enable);
int asb_components_stream_into(asb_ctx* ctx, double* pinned_host, int64_t count);
int asb_host_alloc(int64_t count, double** out);
int asb_host_free(double* p);
int asb_components_pinned(asb_ctx* ctx, double** comps_pinned_out);
/* installs a caller-assigned basis (host, K x n_loc x 3) as the device-resident one */
int asb_components_upload(asb_ctx* ctx, const double* comps_host, int64_t K);

/* ------------------------------------------------ geodesics on the device (optional) ---- */
/* GeodesicDistanceComputation, utils/support.py:139-208, with the two SuperLU solves replaced by
 * Jacobi-PCG for up to 64 sources at a time.  Operators (host CSR, int32 indices), assembled by the caller
 * from the mesh: heat = A - tL, lap = -L (both n x n, SPD / SPSD), grad (m3 x n), div (n x m3), and the
 * diagonals of heat and lap. */
int asb_geodesic_setup(asb_ctx* ctx, int n, int m3, const int* heat_rp, const int* heat_ci, const double* heat_v,
                       const int* lap_rp, const int* lap_ci, const double* lap_v, const int* grad_rp,
                       const int* grad_ci, const double* grad_v, const int* div_rp, const int* div_ci,
                       const double* div_v, const double* heat_diag, const double* lap_diag);
/* Two-level preconditioner for the sparse (PCG) mode -- what lets it scale past the dense mode's 46 000 vertices: agg (n) =
 * aggregate (0 .. nc-1) of every vertex, agg_ptr / agg_mem its CSR form, heat_c / lap_c (host, nc x nc, SPD) the coarse
 * operators P^T (A - tL) P and P^T (-L) P + gauge with P the piecewise-constant prolongation; they are inverted on the
 * device and every PCG step of the POISSON system adds P Ac^-1 P^T r to the Jacobi step.  The HEAT system is solved by
 * (damped, heat_omega in (0, 1]) Jacobi sweeps from zero instead: its solution spans many orders of magnitude and the
 * method needs every component to relative accuracy, which a sweep that only adds non-negative terms delivers and a Krylov
 * method does not.  Quasi-uniform meshes only (the sweep's rate is 1 - min area / (area + t sum w)); otherwise the solve
 * fails with ASB_ERR_NUMERIC and the host backend is the way. */
int asb_geodesic_coarse_setup(asb_ctx* ctx, int nc, const int* agg, const int* agg_ptr, const int* agg_mem,
                              const double* heat_c, const double* lap_c, double heat_omega);
/* distances (min-shifted, :206) from nsrc <= 64 sources: out host (nsrc, n); tol = relative residual of the
 * CG solves; iters (optional, 2 ints) = iterations of the heat and the Poisson solve */
int asb_geodesic_solve(asb_ctx* ctx, const int64_t* sources, int nsrc, double tol, double* out, int* iters);
/* Dense mode (after asb_geodesic_setup): the counterpart of the reference's two SuperLU factorisations
 * (utils/support.py:170-171) for meshes whose N x N matrices are cheap in HBM (N <= 46 000: 2 x 17 GB).  Inverts
 * (A - tL) and the gauge-fixed -L once on the device (blocked Gauss-Jordan on f64 MFMA); asb_geodesic_solve then
 * needs no iteration: the heat step is a column gather, the Poisson step one dense product.  tol / iters unused. */
int asb_geodesic_dense_setup(asb_ctx* ctx);
/* Slab mode (round 4): a DIRECT factorisation of both systems as block-tridiagonal matrices over breadth-first slabs of the mesh
 * graph -- what the reference's two splu factorisations (utils/support.py:170-171) are for meshes beyond the dense inverses'
 * 46 000 vertices and for badly graded ones (no iteration, no convergence question).  slab_ptr (nslab + 1): slab boundaries in a
 * PERMUTED numbering in which every edge joins vertices of the same or of adjacent slabs; perm_of_vertex (n): vertex ->
 * permuted index; heat / lap: A - tL and -L as CSR in that numbering (host). */
int asb_geodesic_bt_setup(asb_ctx* ctx, int nslab, const int* slab_ptr, const int* perm_of_vertex, const int* heat_rp,
                          const int* heat_ci, const double* heat_v, const int* lap_rp, const int* lap_ci, const double* lap_v);
/* support='local' step without a host round trip (posComponents.py:87-105, dense geodesics): reads the vertex
 * asb_deflate_pick chose for component k on the device, solves its distance field, forms
 * s = 1 - (clip(phi, dmin, dmax) - dmin) / (dmax - dmin) (:61-64) for this shard and applies the deflation. */
int asb_deflate_apply_geodesic(asb_ctx* ctx, int64_t k, double dmin, double dmax);
/* Distance fields kept on the device for SPLOCS (posComponents.py:158-165 asks for the fields of the K centres in every
 * outer iteration): solves the fields of nsrc (<= 64) new sources and appends them to the context's cache (4096 slots);
 * *slot0 = slot of the first.  ASB_ERR_LIMIT when full; asb_geodesic_cache_clear empties the cache (buffers stay). */
int asb_geodesic_cache_add(asb_ctx* ctx, const int64_t* sources, int nsrc, double tol, int64_t* slot0);
int asb_geodesic_cache_clear(asb_ctx* ctx);

/* ------------------------------------------------ snapshot ingest --------------- */
/* align, utils/process.py:235-250 (find_rbm_procrustes :210-234 + transform :196-208 per frame): every
 * frame is moved onto frame 0 by the rigid-body motion of the orthogonal Procrustes problem.
 * frames: host (F, N, 3) float64, overwritten; T_out: optional host (F, 4, 4) matrices. */
int asb_align_frames(asb_ctx* ctx, double* frames, int64_t F, int64_t N, int rigid, double* T_out);

/* ------------------------------------------------ constraint-projection bases (config 5) ---- */
/* compute_pod_for_vectorized_nonlinear_snapshots_tensor, snapbases/constraintsComponents.py:298-320:
 * the reference takes svd(A), A = (3ep x F).  asb_pod_gram: G = A^T A (F x F) of this shard (f64 MFMA)
 * into G_dev (caller's device buffer, all-reduced over ranks by the caller) and/or G_host.
 * The F x F eigen-problem is solved by the caller (LAPACK); asb_pod_basis then forms the K leading left
 * vectors  comps[i] = A V[:, i] / sigma[i]  (V host F x K, sigma host K) as the device-resident basis. */
int asb_pod_gram(asb_ctx* ctx, double* G_dev, double* G_host);
int asb_pod_basis(asb_ctx* ctx, const double* V, const double* sigma, int64_t K);
/* Rayleigh-Ritz refinement of the POD basis: B = Q^T A (K x F, this shard's partial sum) for the device-resident
 * (orthonormalised) basis Q, into B_dev (to be all-reduced) and/or B_host.  The SVD of the small B, taken from A
 * itself, restores the eps * sigma_0 / sigma_k accuracy of the reference's `svd` (:307) that the Gram route
 * (eps * (sigma_0 / sigma_k)^2) loses on weak components; the rotation is applied with asb_components_transform. */
int asb_pod_project(asb_ctx* ctx, double* B_dev, double* B_host);
/* keeps the first K components of the device-resident basis (drops the oversampling vectors of the refinement) */
int asb_components_truncate(asb_ctx* ctx, int64_t K);

/* The F x F symmetric eigen-problem of the POD (the `svd` of constraintsComponents.py:307 in Gram form) on the
 * device.  asb_sym_tridiag: Householder tridiagonalisation A = Q T Q^T of the n x n symmetric matrix A_dev
 * (row-major, both triangles; NULL = the Gram matrix asb_pod_gram left in the context).  A is overwritten with
 * the reflectors; d_host (n) / e_host (n-1) receive T's diagonal / off-diagonal.  Ordered reductions only:
 * bit-identical on every rank.  The caller solves the tridiagonal problem (O(n^2)).
 * asb_sym_backtransform: V = Q Z for k eigenvectors Z of T (host, n x k row-major) -> V_host (n x k). */
int asb_sym_tridiag(asb_ctx* ctx, double* A_dev, int64_t n, double* d_host, double* e_host);
int asb_sym_backtransform(asb_ctx* ctx, const double* A_dev, int64_t n, const double* Z_host, int64_t k, double* V_host);
/* The same eigen-problem with NOTHING on the host (n >= 3): tridiagonalisation, then all eigenvalues of T by bisection
 * on Sturm counts and its k leading eigenvectors by inverse iteration (csrc/asb_smalldense.hip), then the
 * back-transformation.  lam_host (n): all eigenvalues, descending; the k vectors stay on the device for
 * asb_pod_basis_dev (V_host, optional n x k row-major, receives a copy); *n_bad (optional): inverse iterations that missed
 * their growth criterion.  Vectors of eigenvalues closer than ~eps |T| / 1e-5 are accurate as a SPAN, not one by one
 * (no re-orthogonalisation inside clusters): the POD follows with a Rayleigh-Ritz step on the snapshot matrix. */
int asb_sym_eig_topk(asb_ctx* ctx, double* A_dev, int64_t n, int64_t k, double* lam_host, double* V_host, int64_t* n_bad);
/* asb_pod_basis from the eigen-pairs asb_sym_eig_topk left on the device: comps[i] = A V[:, i] / sqrt(lam[i]), i < K */
int asb_pod_basis_dev(asb_ctx* ctx, int64_t K);
/* Rayleigh-Ritz rotation on the device: singular values (S_host, K, descending) and left vectors U_B of the (all-reduced)
 * K x F matrix B = Q^T A (B_dev, or the context's from asb_pod_project; overwritten) by one-sided Jacobi on its rows;
 * basis <- Q U_B.  Replaces the small host SVD between asb_pod_project and asb_components_transform. */
int asb_pod_rotate(asb_ctx* ctx, double* B_dev, double* S_host);
/* One step of subspace iteration from the Rayleigh-Ritz result: basis <- A V Sigma^-1 with the right Ritz vectors asb_pod_rotate
 * left in B (even K, F and row count).  Followed by CholeskyQR2 + asb_pod_project + asb_pod_rotate again it removes most of what the
 * Gram route's eps (sigma_0 / sigma_k)^2 leaves OUTSIDE the Ritz subspace of the weak vectors (constraintsComponents.py:307: the
 * reference's gesdd has no such loss). */
int asb_pod_power(asb_ctx* ctx, const double* B_dev);
/* The POD in LEVELS: singular values below ~1e-8 sigma_0 are invisible in the Gram matrix of A (where the reference's gesdd on A
 * itself still returns vectors, constraintsComponents.py:307-316) but not in the Gram matrix of A_2 = A - U_1 (U_1^T A).
 * asb_pod_deflate_begin(ctx, B_dev, keep): the first `keep` rows of the basis are kept (behind what earlier levels kept) and the
 * context's snapshots become A_2 (a second buffer; even `keep`, F and row count); the POD entry points then work on A_2.
 * asb_pod_deflate_end(ctx, last): the snapshots are the original ones again, the basis is [kept rows of all levels ; the first
 * `last` rows of the current basis].  Ingesting new snapshots ends an open level: the kept rows are dropped and a later
 * asb_pod_deflate_end is refused. */
int asb_pod_deflate_begin(asb_ctx* ctx, const double* B_dev, int64_t keep);
int asb_pod_deflate_end(asb_ctx* ctx, int64_t last);
/* constProj_basis_type 'pod' (compute_pod_for_nonlinear_snapshots_tensor, :274-294): one SVD per (constraint row, coordinate)
 * slice of the snapshots -- e x F matrices -- by Gram matrix + device eigen-solver; the K leading left vectors of every
 * slice become the device-resident basis (K, e p, 3).  The reference does this in float32 with torch on the CPU. */
int asb_pod_slices(asb_ctx* ctx, int p, int64_t K);
/* The same per-slice POD in phases, for rows sharded over ranks in whole constraints (v0 and n_loc multiples of p); slice
 * s = 3 p_i + d.  asb_pod_slice_grams: this shard's partial Gram matrices (F x F each) of slices s0 .. s0 + ns - 1 into G_dev
 * (ns x F x F; the caller all-reduces them).  asb_pod_slice_eig: the owner's eigen-solve of one all-reduced Gram matrix
 * (G_dev, overwritten) -> V S^-1 (F x K row-major) into VS_dev and the refusal flag (1.0: fewer than K singular values above
 * 1e-7 of the largest, else 0.0) into status_dev[0].  asb_pod_slices_basis: the shard's basis rows (K, n_loc, 3) from
 * VS_all_dev = the all-reduced (3p, F, K) vectors followed by the 3p flags; a set flag fails as asb_pod_slices does.  On one
 * rank the three phases give asb_pod_slices' basis bit for bit. */
int asb_pod_slice_grams(asb_ctx* ctx, int p, int s0, int ns, double* G_dev);
int asb_pod_slice_eig(asb_ctx* ctx, int64_t K, double* G_dev, double* VS_dev, double* status_dev);
int asb_pod_slices_basis(asb_ctx* ctx, int p, int64_t K, const double* VS_all_dev);
/* asb_qr_apply with ONE Cholesky factor of the sum of the three Gram matrices for all three slices: the basis becomes
 * orthonormal as (3 n)-vectors (the Q of the Rayleigh-Ritz step).  Any K. */
int asb_qr_apply_joint(asb_ctx* ctx, const double* G_dev);
/* :421-428 / :440-443 the reference also restores the snapshot tensor:
 * X <- (X * inv_scale + mean) * rowscale[v]   (rowscale host n_loc or NULL) */
int asb_snapshots_affine(asb_ctx* ctx, double inv_scale, int add_mean, const double* rowscale);
/* :430-433 `qr(comps[:,:,l].T, mode='economic')[0].T`: one CholeskyQR pass per dimension with the
 * Gram matrices of asb_orth_gram (NULL: the context's).  Call gram/apply twice (CholeskyQR2).  K <= 128: one block's
 * LDS; larger K (the reference's configurations use 200 ... 1000): blocked Cholesky + inverse, csrc/asb_smalldense.hip. */
int asb_qr_apply(asb_ctx* ctx, const double* G_dev);
/* deim, :797-860, device half: residual r = V[:, :k] coef - v_k per dimension and its arg-max over this
 * shard (global row index).  coef: host (3, k), NULL for k = 0.  The k x k interpolation solves stay with
 * the caller (numpy lstsq, as in the reference :829), fed by asb_deim_row. */
int asb_deim_step(asb_ctx* ctx, int64_t k, const double* coef, int64_t* idx_out, double* val_out);
/* deim (:797-860) entirely on the device, for a basis whose rows are all on this rank: Pt_out (K) = the interpolation rows in
 * order; maxabs_out (K) = the largest |residual| entry of each step (the reference stops with "zero residual" when
 * np.allclose(r, 0), i.e. <= 1e-8); the k x k systems are solved through a bordered inverse carried on the device and
 * verified -- *solve_failed != 0 means a check failed (or no row could be named because the coefficients were not finite)
 * and the caller should fall back to asb_deim_step + lstsq (:829).  Every Pt_out entry is a row of the basis either way.
 * ASB_ERR_LIMIT, before anything is allocated or launched, when (11 K + 64) doubles exceed the device's LDS per block. */
int asb_deim_run(asb_ctx* ctx, int64_t* Pt_out, double* maxabs_out, int* solve_failed);
/* deim_blocksForm (:733-795) / geom_block_form_utilizing_differential_operator (:619-731, error in the constraint space):
 * residual of block k (p basis vectors) with the interpolation coefficients coef (host, 3 x (k p) x p; NULL at k = 0);
 * per-row energies into the context (arg-max over rows / constraints: asb_deflate_block_argmax with group 1 / p);
 * *maxabs_out = largest |r| entry (np.allclose(r, 0) test of :771). */
int asb_deim_block_residual(asb_ctx* ctx, int64_t k, int p, const double* coef, double* maxabs_out);
/* first maximum over this shard of the sums of p consecutive per-row energies held by the context (global block index) */
int asb_energy_block_argmax(asb_ctx* ctx, int p, int64_t* block_out, double* val_out);
/* V[gidx, :, :] -> row_out (K, 3); returns 1 (and writes nothing) when another rank owns gidx */
int asb_deim_row(asb_ctx* ctx, int64_t gidx, double* row_out);

/* ------------------------------------- reconstruction errors / held-out projection ---- */
/* posComponents.test_convergence, snapbases/posComponents.py:192-249, without forming a reconstruction: ONE read of the
 * tensor per call.  which 0: the training tensor X with the greedy weights (W of the deflation) and the device-resident
 * basis, tensordot(weigs[:, :k], comps[:k]) (:196-197); which 1: the held-out tensor of asb_heldout_upload with the
 * least-squares prefix weights of asb_heldout_factor.  ks: S strictly increasing sweep points 0 <= k_1 < ... <= K
 * (S <= 1024).  This shard's partial values: sums_out (S x 3) sum_{f,v} (T_d - R_k,d)^2 per axis (:217-237),
 * max_out (S) max |T - R_k| (:239-249), norms_out (4) sum T_x^2, sum T_y^2, sum T_z^2 and the SIGNED max T (np.max(f)).
 * Deterministic (fixed-order reductions, no atomics).  Any output pointer may be NULL. */
int asb_recon_sweep(asb_ctx* ctx, int which, const int64_t* ks, int64_t S, double* sums_out, double* max_out,
                    double* norms_out);
/* The test animation of posSnapshots.py:119-121 (test_verts), host (F, N_glob, 3): vertices [v0, v0+n_loc) of this shard
 * (the training shard), transformed exactly as the training tensor was (:82, :168, :172): times massL[v0+v] when massL !=
 * NULL, minus the TRAINING mean row when subtract != 0, times the training pre_scale_factor.  F may differ from the
 * training F. */
int asb_heldout_upload(asb_ctx* ctx, const double* Y, int64_t F, int64_t N_glob, int64_t v0, int64_t n_loc,
                       const double* massL, int subtract, double pre_scale_factor);
/* P = Y C^T (F x K) and G = C C^T (K x K) of this shard for the current basis, into the caller's device buffers (to be
 * all-reduced over ranks) or into the context when NULL -- the products of asb_splocs_gram. */
int asb_heldout_gram(asb_ctx* ctx, double* P_dev, double* G_dev);
/* With the (summed) P, G (NULL: the context's own): G = L L^T on the host, Q = L^-1 C and Z = P L^-T on the device, so
 * that the projection of Y onto span(c_0 .. c_k-1) is Z[:, :k] Q[:k] for every prefix k.  A pivot <= 3 N eps trace(G)
 * marks a component dependent on the earlier ones: its row of Q and column of Z are zero (span and errors unchanged).
 * n_dropped (optional): how many were dropped. */
int asb_heldout_factor(asb_ctx* ctx, const double* P_dev, const double* G_dev, int64_t* n_dropped);
/* the least-squares weights of the held-out frames on the components, W = Z L^-1 (host, F x K; 0 for dropped ones) */
int asb_heldout_weights(asb_ctx* ctx, double* W_out);

/* ----------------------------- interpolation-error sweeps of constraint bases ---- */
/* The row analogue of asb_deim_row: frames[:, gidx, :] of this shard, gathered on the device.  which 0: the prepared
 * snapshots X (nonlinearSnapshots.snapTensor, post-processing included); 1: the held-out frames of asb_heldout_upload
 * (test_snapTensor, nonlinear_snapshots.py:115-122, uploaded raw: massL NULL, subtract 0, scale 1).  out (host, n x F x 3);
 * a row another rank owns is 0 there and owned_out[i] = 0 (owned_out optional), so the rows of all ranks sum to frames[:, gidx]. */
int asb_rows_gather(asb_ctx* ctx, int which, const int64_t* gidx, int64_t n, double* out, int* owned_out);
/* nl_reduction_tests.run_geom_tests (generate_figures/nl_reduction_tests.py:117-225) for S <= 64 sweep points without forming a
 * reconstruction: per point s, the geom_constructed reconstruction (constraintsComponents.py:489-521) from rp[s] basis vectors,
 * V[:, :rp, l] C_{s,l} with C_{s,l} = M_{s,l} B_l[:npt[s]], formed on the device, and its errors against the tensor of `which`
 * (as in asb_rows_gather).  M (host): per s in order, 3 x rp[s] x npt[s] doubles, M_{s,l} = (A^T A)^-1 A^T, A = V[Pt_s, :rp, l]
 * (:515-519); B (host, nb x F x 3): the rows at the interpolation points, nb >= npt[s].  This shard's partial values: sums_out
 * (S x 3) sum (f - rec)^2 per axis (:524-545), max_out (S) max |f - rec| (:547-556), norms_out (4) sum f_x^2, sum f_y^2,
 * sum f_z^2 and the SIGNED max f (np.max(f)).  One read of the tensor per call; deterministic (fixed-order reductions, no
 * atomics).  Any output pointer may be NULL. */
int asb_interp_sweep(asb_ctx* ctx, int which, const int64_t* rp, const int64_t* npt, int64_t S, const double* M, const double* B,
                     int64_t nb, double* sums_out, double* max_out, double* norms_out);

/* ------------------------------------------------- on-mesh accuracy maps ---- */
/* compute_accuracy (generate_figures/onMesh_accuracyMeasures.py:61-151) on the resident tensor, in world space:
 * x = (T / psf + mean) / massL_v of the tensor, x_r the same of R_r = A[:, :r] B[:r] (A, B as in asb_recon_sweep).
 * asb_onmesh_mesh: the triangles (host, n_tris x 3) and the vertex-star CSR -- star_ptr (n_loc + 1) offsets, star_tri
 * (3 n_tris) the incident triangles of each vertex in increasing triangle number, one entry per corner -- of the WHOLE mesh:
 * v0 = 0 and n_loc = N_glob (normals across vertex shards are not built).  Every index is checked; kept until the next call. */
int asb_onmesh_mesh(asb_ctx* ctx, const int64_t* tris, int64_t n_tris, const int64_t* star_ptr, const int64_t* star_tri,
                    int64_t v0, int64_t n_loc);
/* One reconstruction of r components over the frames range(f0, f1, fj) (n_sel of them), `which` as in asb_recon_sweep.
 * inv_massL (host, N_glob, or NULL): 1 / massL; add_mean != 0: the mean row is added back; psf: the scale the tensor was
 * multiplied by (1 when not standardised); denom: sqrt(3 (f1 - f0) N_glob) (:70).  This shard's values:
 *   accum_norm_out (n_loc)   sum_f frame_err[f, v], frame_err = |x - x_r|^2 / |x|^2 / denom (:116, :120)
 *   mesh_num_out, mesh_den_out (n_sel)   sum_v |x - x_r|^2 and sum_v |x|^2 of each frame (:117 = sqrt(num / den) / denom)
 *   accum_angle_out (n_loc)  sum_f angle[f, v] in degrees between the area-weighted per-vertex normals (sum of the incident
 *                            triangles' (b - a) x (c - a), cosine clipped to [-1, 1]) of x and x_r (:73-90, :122-125);
 *                            only with want_normals != 0, which needs asb_onmesh_mesh
 *   stats_out (10)           accum_norm min, sum, max; frame_err min, max; accum_angle min, sum, max; angle min, max
 *                            (NaN-propagating like numpy; the sum of a map is the sum of its accumulated vector)
 *   frame_err_out, angle_out (n_sel x n_loc, may be NULL)   the maps themselves.
 * One read of the tensor for the error pass; the normal pass runs in chunks of frames through a bounded scratch.
 * Deterministic (fixed-order reductions, no atomics).  Any output pointer may be NULL. */
int asb_onmesh_run(asb_ctx* ctx, int which, int64_t r, int64_t f0, int64_t f1, int64_t fj, int want_normals,
                   const double* inv_massL, int add_mean, double psf, double denom, double* accum_norm_out,
                   double* mesh_num_out, double* mesh_den_out, double* accum_angle_out, double* stats_out,
                   double* frame_err_out, double* angle_out);

/* ------------------------------- constraint projections of resident positions ---- */
/* The per-element projections `get_pi` of projective_dynamics/Constraint_projections.py for every frame of the resident
 * position tensor, written in the layout of the simulator's stacked_p (Simulators.py:655-724).  One rank: v0 = 0 and
 * n_loc = N_glob.  kind: 0 edge_spring (p = 1; idx n x 2; table n x 1: rest length), 1 tris_strain (p = 2; idx n x 3; table
 * n x 10: the 3 x 2 tangent frame P, then the 2 x 2 DmInv, both row-major), 2 tets_strain and 3 tets_deformation_gradient
 * (p = 3; idx n x 4; table n x 9: DmInv row-major), 4 verts_bending (p = 1; idx n x 1: the constrained vertices; table n x 5:
 * rest mean-curvature norm, averaged triangle normal, dot_with_normal -- followed by one weight per star edge; star_ptr
 * (n + 1) and star_idx (the neighbour v2 of each star edge, in the reference's edge order) are needed for this kind only).
 * All arrays on the host.  Every index is checked against the vertices of the tensor; kept until the next call. */
int asb_cproj_setup(asb_ctx* ctx, int kind, int64_t n_elem, const int64_t* idx, const double* table, const int64_t* star_ptr,
                    const int64_t* star_idx);
/* The projections of the frames range(f0, f1, fj) (n_sel of them) of the training (which 0) or held-out (1) tensor, from
 * world positions x = (T / psf + mean) / massL_v formed as asb_onmesh_run forms them (same arguments).  sigma_min / sigma_max:
 * the clamp of the two strain kinds.  out_dev: caller-owned DEVICE memory, (n_sel, n_elem p, 3) doubles.  A zero-length edge
 * writes NaN.  Deterministic: no atomics, sub-ranges equal the matching slices of a full run bit for bit.  Returns after the
 * stream has drained. */
int asb_cproj_run(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                  double sigma_min, double sigma_max, double* out_dev);
/* The constraint forces b[f] = S^T p(q_f) of the same frames for the kind of the preceding asb_cproj_setup: the term of that
 * kind in the global step's right-hand side (get_sum_ST_p, Simulators.py:643-724), without forming p at full size.  The first
 * ten arguments are those of asb_cproj_run.  S^T: HOST CSR with n_rows = the tensor's vertices, columns = rows of the stacked
 * projections (< n_elem p), strictly ascending in every row; it is checked before use.  out_dev: caller-owned DEVICE memory,
 * (n_sel, n_rows, 3) doubles.  accumulate 0: every entry is written (0.0 where a vertex's row is empty); 1: added to what is
 * there.  chunk_frames: frames per pass (rounded up to a multiple of 16; 0 or too large: the most a 256 MB scratch of
 * (3 n_elem p) rows holds).  Deterministic: no atomics, every entry is summed by one thread over ascending columns, so
 * sub-ranges, repeats and any chunk_frames give the same bits.  Returns after the stream has drained. */
int asb_cforce_run(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                   double sigma_min, double sigma_max, int64_t n_rows, const int64_t* indptr, const int64_t* indices,
                   const double* data, int accumulate, int64_t chunk_frames, double* out_dev);

/* ------------------------------- DEIM-reduced constraint forces and their error ---- */
/* The reduced constraint term of the reference's simulator, b~_d = (S^T V_d) H_d P^T p_d per coordinate d with
 * H_d = (A^T A + la_d I)^-1 A^T, A = P^T V_d (Simulators.py:157-255 prepare_reduced_group / prepare_reduced_verts_bending,
 * :366-399 get_group_reduced_term), for frames of the resident position tensor.  One rank: v0 = 0 and n_loc = N_glob.
 * asb_rforce_operator: S^T as a HOST CSR (n_rows = the tensor's vertices, columns < v_rows strictly ascending in every row,
 * checked as asb_cforce_run checks it) and the basis V (host, v_rows x mp x 3).  Forms M_d = S^T V_d (three n_rows x mp
 * matrices) on the device, every entry summed by one thread over the row's ascending columns; no dense S^T is formed.  Kept
 * until the next call; drops the solver. */
int asb_rforce_operator(asb_ctx* ctx, int64_t n_rows, const int64_t* indptr, const int64_t* indices, const double* data,
                        int64_t v_rows, int64_t mp, const double* V);
/* The solver of the next asb_rforce_run calls: H (host, 3 x r x npt), r <= mp -- the first r columns of the operator are
 * used -- and per interpolation point the row of the SAMPLED elements' stacked projections it keeps (host, npt; row
 * i p + l is row l of the i-th element handed to asb_cproj_setup). */
int asb_rforce_solver(asb_ctx* ctx, int64_t r, int64_t npt, const double* H, const int64_t* rows);
/* b~ of the frames range(f0, f1, fj) after asb_cproj_setup was called with ONLY the sampled elements: their projections
 * (the arithmetic of asb_cproj_run, first ten arguments as there), coef_d = H_d p_d[rows] (r x n_sel), b~_d = M_d coef_d by
 * an f64 MFMA kernel whose contraction is never split.  out_dev: caller-owned DEVICE memory, (n_sel, n_rows, 3) doubles;
 * accumulate 0: every entry is written, 1: added to what is there.  The cost depends on npt, r, n_rows and n_sel only.
 * Deterministic: no atomics, every entry a fixed-order sum; repeats, accumulate onto zeros and sub-ranges give the bits of the
 * matching slices of a full run.  Returns after the stream has drained. */
int asb_rforce_run(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                   double sigma_min, double sigma_max, int accumulate, double* out_dev);
/* Banks: the context holds ASB_RFORCE_BANKS independent sets of what the calls above and asb_hyper_operator make -- per bank the
 * operator S^T V (3 mpp Np doubles), the solver H (3 r npt doubles) with its rows (npt ints), the coefficient scratch of one
 * chunk of frames (3 rpp cw doubles), A^-1 S^T V with its valid mark (3 mpp Np doubles) and its touched columns Gt_c (3 mpp N_t
 * doubles); a bank that was never addressed holds nothing.  A bank that was addressed KEEPS its buffers, whichever bank is
 * current, until a later call that addresses it sizes them anew or asb_destroy frees them: nothing releases the banks that a
 * solve no longer uses.  asb_rforce_bank selects the set that asb_rforce_operator,
 * asb_rforce_solver, asb_rforce_run and asb_hyper_operator address from now on, and that a reduced asb_pdsolve_slot binds.  Bank
 * 0 is current in a new context.  bank outside 0 .. ASB_RFORCE_BANKS - 1: ASB_ERR_ARG, nothing changed.  Host work only. */
#define ASB_RFORCE_BANKS 8
int asb_rforce_bank(asb_ctx* ctx, int bank);
/* The reference's error metrics (constraintsComponents.py:524-556) of b against a, both DEVICE tensors (F, N, 3): sums_out (3)
 * sum (a - b)^2 per axis, max_out (1) max |a - b|, norms_out (4) sum a_x^2, sum a_y^2, sum a_z^2 and the SIGNED max a,
 * per_frame_out (F x 2) per frame [sum (a - b)^2, sum a^2] over its N x 3 entries.  Fixed-order reductions, no atomics; a
 * NaN propagates through the sums as in asb_recon_sweep.  Any output pointer may be NULL. */
int asb_force_diff(asb_ctx* ctx, const double* a_dev, const double* b_dev, int64_t F, int64_t N, double* sums_out, double* max_out,
                   double* norms_out, double* per_frame_out);

/* ------------------------------- global step of projective dynamics ---- */
/* q = A^-1 rhs for A_N = M / h^2 + sum_i w_i S_i^T S_i (Simulators.py:117-145, :508-526): the reference's 3N x 3N matrix is
 * kron(A_N, I_3), so one N x N matrix serves the three coordinates.  One rank: v0 = 0 and n_loc = N_glob.
 * asb_gstep_setup: A_N as a HOST CSR (n = the tensor's vertices rows and columns, columns strictly ascending in every row),
 * checked before use: positive diagonal, symmetric pattern, values symmetric to 1e-12 of the row's largest entry.  It is
 * scattered into a dense matrix padded to a multiple of 32 by an identity block and inverted in place on the device (blocked
 * Gauss-Jordan, f64 MFMA); the inverse belongs to the context until the next set-up or asb_destroy.  n <= 46000 (17 GB),
 * larger n: ASB_ERR_LIMIT, checked before anything else is read.  resid_out (optional): max |A (A^-1 u) - u| for u = 1, A
 * applied as the sparse matrix, fixed summation order. */
int asb_gstep_setup(asb_ctx* ctx, int64_t n, const int64_t* indptr, const int64_t* indices, const double* data, double* resid_out);
/* out[f, m, d] = sum_n rhs[f, n, d] A^-1[n, m]: both caller-owned DEVICE tensors (n_frames, n, 3), frame-major, neither is
 * transposed and they must not overlap.  f64 MFMA, the three coordinates share every tile of A^-1; the contraction is never
 * split, every entry is one accumulator summed over ascending n: no atomics, repeats and frame sub-ranges give identical bits.
 * Every entry of out is written.  Returns after the stream has drained. */
int asb_gstep_run(asb_ctx* ctx, const double* rhs_dev, int64_t n_frames, double* out_dev);
/* rhs[f, n, d] += diag[n] s_f[n, d] for the frames range(f0, f1, fj) of the training (which 0) or held-out (1) tensor, from
 * the world positions x of asb_cproj_run (arguments two to eight as there; no element set-up is needed).
 * diag (host, n): masses / h^2; acc3 (host, 3): h^2 g.  mode 0: s_f = x_f + acc; mode 1: s_f = 2 x_f - x_{f-1} + acc, f - 1
 * the TENSOR's previous frame (at frame 0: x_0), the explicit step of Simulators.py:494-495 with the velocity of :531.
 * rhs_dev: caller-owned DEVICE memory (n_sel, n, 3), read and written entry by entry.  Returns after the stream has drained. */
int asb_gstep_inertia(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                      const double* diag, int mode, const double* acc3, double* rhs_dev);
/* test hook: the n x n block of the context's A^-1 (row-major) to the host; refused (ASB_ERR_ARG) under the slab factor */
int asb_test_gstep_inverse(asb_ctx* ctx, double* out_host, int64_t n);

/* ------------------------------- global step: the block-tridiagonal slab factor (asb_gslab.hip) ---- */
/* The second solver of the global step, for any n that fits the memory.  The context holds EITHER the explicit inverse of
 * asb_gstep_setup OR this factor (or the position subspace of asb_gsub_setup below): each set-up releases the others and
 * invalidates the operator of asb_hyper_operator.  With the
 * factor held, asb_gstep_run, asb_pdsolve_begin / _iterate, asb_hyper_operator and asb_hyper_iterate apply A^-1 through it;
 * asb_pdsolve_iterate with a history and asb_test_gstep_inverse are refused (ASB_ERR_ARG).
 * asb_gslab_setup: A_N as the HOST CSR of asb_gstep_setup, with that entry's checks, plus a slab plan (projections.slab_plan):
 * order (n) = permuted index -> vertex, a permutation; slab_ptr (nslab + 1) = slab boundaries in the permuted numbering,
 * ascending from 0 to n; no entry of A may couple slabs more than one apart.  Each violation is ASB_ERR_ARG; the counts are
 * judged before anything behind a pointer is read.  ASB_ERR_LIMIT: padded rows past 32-bit indices, or a slab of more than
 * 8192 vertices.  S_0 = A_00, S_k = A_kk - C_k S_{k-1}^-1 C_k^T (C_k = A_{k,k-1}) are formed and inverted on the device (the dense
 * layer's GEMM and SPD inverse); only the S_k^-1 are kept, padded to multiples of 16: sum sp_k^2 doubles.  A Schur complement
 * that is not positive definite: ASB_ERR_NUMERIC, no solver is left.  resid_out (optional): max |A (A^-1 u) - u| for u = 1
 * through the sweep and the sparse A.
 * The sweep: forward u_k = S_k^-1 (b_k - C_k u_{k-1}), backward x_k = u_k - S_k^-1 (C_{k+1}^T x_{k+1}), all columns at once, one
 * sparse and one f64-MFMA product per slab and direction in stream order.  No contraction is split between blocks and
 * nothing is atomic: an entry does not depend on the columns around it, on chunk_frames or on a repeat. */
int asb_gslab_setup(asb_ctx* ctx, int64_t n, const int64_t* indptr, const int64_t* indices, const double* data, int64_t nslab,
                    const int64_t* slab_ptr, const int64_t* order, double* resid_out);
/* counts_out (4): slabs, largest padded slab, padded rows of the work matrix, doubles held by the factor */
int asb_gslab_info(asb_ctx* ctx, int64_t* counts_out);
/* test hook: out_host (n, w) = A^-1 rhs_host (n, w) through the sweep; any w >= 1, host arrays (they may be the same) */
int asb_test_gslab_solve(asb_ctx* ctx, const double* rhs_host, int64_t w, double* out_host);
/* timing hook: ms_out (2) = best of three of the sweep's product kernel and of asb_gemm_nn on the same (sp x sp) (sp x w) product
 * of zero-filled device buffers; sp a multiple of 16 (<= 8192), w of 64 */
int asb_test_gslab_gemm_time(asb_ctx* ctx, int64_t sp, int64_t w, double* ms_out);

/* ------------------------------- global step in a position subspace q = o + U z (asb_gsub.hip) ---- */
/* The third solver of the global step: per coordinate d the Galerkin step q_d = o_d + U_d (U_d^T A U_d)^-1 U_d^T (rhs_d - A o_d)
 * = o'_d + P_d rhs_d for a basis U_d (n x r) of full column rank and an origin o (the reference's reduced_position branch,
 * Simulators.py:38-41, :144-155).  The context holds exactly ONE of the explicit inverse, the slab factor and this subspace:
 * each set-up releases the other two and invalidates the operator of asb_hyper_operator in every bank.  With the subspace held,
 * asb_gstep_run and the product of asb_pdsolve_iterate apply the AFFINE map, c of asb_hyper_iterate is o' + P ms, and
 * asb_hyper_operator forms G = P S^T V (the LINEAR part); asb_pdsolve_iterate with a history is refused (ASB_ERR_ARG).
 * asb_gsub_setup: A_N as the HOST CSR of asb_gstep_setup with that entry's checks; Qt_host (3, r, n) = U_d^T (any basis of the
 * span; the host passes orthonormal columns, projections.subspace_basis); origin_host (n, 3).  n < 1, r < 1 or a NULL pointer:
 * ASB_ERR_ARG, judged on the counts before anything behind a pointer is read; r > n and values that are not finite:
 * ASB_ERR_ARG; r > 8192: ASB_ERR_LIMIT.  A U_d by the sparse x dense kernel of asb_rforce_operator, U_d^T (A U_d) and its SPD
 * inverse (padded to a multiple of 16 by an identity block) by the dense layer; not positive definite: ASB_ERR_NUMERIC, no
 * solver is left.  Kept: U^T (3, rp, Np), W^T = U (U^T A U)^-1 (3, Np, rq), the inverses, o' (rp, rq: r rounded up to 4 and 16,
 * Np: n to 32), and for the asb_zroll_* entries below U in W's layout (3, Np, rq), o and A o (n, 3).  resid_out (optional): max_d max |U_d^T (A (P_d 1) - 1)| as the device computed it.
 * The map is two f64-MFMA products, Y = W R over all vertices (never split between blocks) and Q = o' + U Y; no atomics: an
 * entry does not depend on the columns around it, on chunk_frames, on the touched set or on a repeat. */
int asb_gsub_setup(asb_ctx* ctx, int64_t n, const int64_t* indptr, const int64_t* indices, const double* data, int64_t r,
                   const double* Qt_host, const double* origin_host, double* resid_out);
/* counts_out (4): r, rq, Np, rp */
int asb_gsub_info(asb_ctx* ctx, int64_t* counts_out);
/* test hook: rhs_host (3 n, w) vertex-major (row 3 v + d), any w >= 1; out_host (3 n, ld), ld = w rounded up to 64, is read and
 * written: columns [0, w) become o' affine + P rhs (affine 0: the linear part), the others come back as they went in */
int asb_test_gsub_apply(asb_ctx* ctx, const double* rhs_host, int64_t w, int affine, double* out_host);
/* test hook: what the set-up left, as it lies on the device; which 0: W^T (3, Np, rq), 1: the inverses (3, rq, rq), 2: o' (n, 3),
 * 3: U^T (3, rp, Np); len = the doubles of out_host (checked) */
int asb_test_gsub_state(asb_ctx* ctx, int which, double* out_host, int64_t len);

/* ------------------------------- roll-outs with the state in z under the position subspace (asb_zroll.hip) ---- */
/* With the subspace of asb_gsub_setup held and EVERY kind reduced, a time step of the hyper-reduced solver is carried in the
 * coordinates z of q = o + U z: per coordinate z' = c_z + sum_k Gz_k coef_k(q at the touched vertices), c_z = kappa + T y + E target,
 * y = 2 z - z_prev.  T, kappa, E and the touched rows of U are formed once per asb_zroll_begin, Gz_k = (U^T A U)^-1 U^T S^T V_k once per
 * asb_zroll_operator; a step reads and writes nothing of size N.  Without a subspace every entry returns ASB_ERR_ARG.
 * asb_gsub_coordinates: out_dev (F', r, 3) = U^T (x_f - o) of the frames range(f0, f1, fj) of the tensor `which` (the leading
 *   arguments of asb_pdsolve_begin), or, with pos_dev != NULL, of the caller's contiguous device tensor (n_frames, n, 3).  The chain
 *   of an entry walks the n vertices in ascending order and is never split.
 * asb_gsub_expand: out_dev (n_frames, n, 3) = o + U z for z_dev (n_frames, r, 3).
 * asb_zroll_operator: Gz of the CURRENT bank from its S^T V (asb_rforce_operator) and the subspace; marked valid, and invalidated
 *   exactly when that bank's operator of asb_hyper_operator is: by every solver set-up (all banks) and by asb_rforce_operator (its own).
 * asb_zroll_begin: the frame arguments, diag = masses / h^2 (n), mode (0: z_prev = z, 1: z_prev from the animation's previous
 *   frame) and acc3 = h^2 g of asb_pdsolve_begin; touched: the n_touched ascending vertices the slots' element set-ups are numbered
 *   in; z_dev, zprev_dev: both NULL, or the state (F', r, 3) of a continuation (mode is then ignored).  Counts are judged before
 *   pointers (ASB_ERR_ARG); more than 65535 * 64 frames: ASB_ERR_LIMIT.
 * asb_zroll_slot: the set-up of the last asb_cproj_setup becomes the next kind, reduced, with the operator and solver of the
 *   current bank (one kind per bank; at most 8).
 * asb_zroll_pins: binds the pins of asb_pins_set; step t = 1, 2, .. from frame f reads row row0 + f + t - 1 of the shift.
 * asb_zroll_steps: n_steps steps of n_iter iterations, all in stream order with ONE drain at the end.  record_every = e > 0: z after
 *   the steps e, 2 e, .. into records_dev (R, F', r, 3).  A stale Gz, a subspace or pins that changed since asb_zroll_begin, and a
 *   row of the shift that does not exist are refused (ASB_ERR_ARG) before anything is launched.  chunk_frames as asb_hyper_iterate.
 * asb_zroll_state: z and z_prev (F', r, 3) after the steps taken so far.
 * Nothing is split between blocks and nothing is atomic: repeats, frame sub-ranges, chunk widths and continuations give the bits
 * of the whole. */
int asb_gsub_coordinates(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                         const double* pos_dev, int64_t n_frames, double* out_dev);
int asb_gsub_expand(asb_ctx* ctx, const double* z_dev, int64_t n_frames, double* out_dev);
/* asb_force_diff(a, b, ..) for b = o + U z with b never stored: a_dev (n_frames, n, 3) and z_dev (n_frames, r, 3) are caller-owned
 * DEVICE tensors, the four outputs mean what they mean in asb_force_diff (any may be NULL), o and U are those of the subspace the
 * context holds.  No subspace, n_frames < 1, a NULL tensor: ASB_ERR_ARG; the frame limit of asb_gsub_expand (ASB_ERR_LIMIT).
 * One kernel forms q~ = o + U z tile by tile with the MFMA chain of asb_gsub_expand -- its bits, whatever the tile, the width or
 * the neighbours -- and consumes it in registers with the per-entry arithmetic of asb_force_diff (e = a - q~, fma onto the sums,
 * fmax of |e| and of the signed a); a is read once, in runs of 96 doubles per 32 vertices and frame, through LDS.  Reductions: a
 * lane adds its entries ascending in the vertex, the four lanes of a frame are combined in a fixed order, a block walks its
 * vertex tiles in ascending order, the blocks' records of a frame are added in ascending vertex order, and the frames by the
 * kernel of asb_force_diff.  No atomics: repeats give identical bits, and a frame's record depends neither on n_frames nor on
 * the frames beside it (the split of the vertices between blocks depends on n alone).  The order over the vertices is not that
 * of asb_force_diff: the sums agree with it to rounding, the two maxima exactly.  Vertices and frames of the padding contribute
 * nothing and no address is formed for them; a NaN propagates through the sums of its frame and axis.
 * Scratch, freed before the call returns: z repacked (3 rq ld doubles, ld = n_frames rounded up to 64), the blocks' records
 * 8 G ld doubles with G = ceil(T / ceil(T / 256)) <= 256 groups of the T = ceil(n / 32) vertex tiles, and 8 (n_frames + 1)
 * doubles of frame records -- at most 2048 ld doubles beside z, never n x n_frames.  Returns after the stream has drained. */
int asb_gsub_expand_diff(asb_ctx* ctx, const double* a_dev, const double* z_dev, int64_t n_frames, double* sums_out, double* max_out,
                         double* norms_out, double* per_frame_out);
int asb_zroll_operator(asb_ctx* ctx);
int asb_zroll_begin(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                    const double* diag, int mode, const double* acc3, int64_t n_touched, const int64_t* touched, const double* z_dev,
                    const double* zprev_dev);
int asb_zroll_slot(asb_ctx* ctx, double sigma_min, double sigma_max);
int asb_zroll_pins(asb_ctx* ctx, int64_t row0);
/* asb_zroll_forces: after asb_zroll_begin and an asb_ext_set WITH a table and WITHOUT a floor (a floor is refused: a clamp on vertex
 * coordinates has no form in z).  Binds the table: Phi_d = W_d (D o fa_d) joins c_z and the touched rows of a step's first iterate take
 * fl(. + fa[row]); step t = 1, 2, .. from frame f reads row row0 + f + t - 1 (a constant table: its one row).  ALL T_s rows are prepared
 * here, once -- what a later asb_zroll_steps reads is not known yet --, by the reduce of asb_gsub.hip, the chain over N never split; at
 * most 65535 rows (ASB_ERR_LIMIT).  A step is two launches longer.  asb_zroll_steps checks the last row it will read before its first
 * launch (ASB_ERR_ARG).  A new asb_zroll_begin drops the binding.  In stream order; the call does not wait. */
int asb_zroll_forces(asb_ctx* ctx, int64_t row0);
int asb_zroll_steps(asb_ctx* ctx, int64_t n_steps, int64_t n_iter, int64_t chunk_frames, int64_t record_every, double* records_dev);
int asb_zroll_state(asb_ctx* ctx, double* z_dev, double* zprev_dev);
/* test hook: the affine product kernel alone, Out = base + sum_s M_s X_s on host arrays.  r rows, w columns, n_seg <= 8 segments of
 * lengths klen[s]; M_host: the (3, r, klen[s]) one behind the other, X_host: the (3, klen[s], w); base_host (3, r, w), or (3, r)
 * broadcast over the columns with bcast; out_host (3, rq, ld), rq = r rounded up to 16 and ld = w to 64: the whole padded result */
int asb_test_zroll_affine(asb_ctx* ctx, int64_t r, int64_t w, int64_t n_seg, const int64_t* klen, const double* M_host, const double* X_host,
                          const double* base_host, int bcast, double* out_host);

/* ------------------------------------------------ projective dynamics: the solver's iterations (asb_pdsolve.hip) ----------- */
/* The local/global loop of Simulators.py:494-526 for the frames range(f0, f1, fj) of the training (which 0) or held-out (1)
 * tensor, every frame an independent solve: q_{k+1} = A^-1 (sum_i S_i^T p_i(q_k) + M / h^2 s_f) with s_f fixed.  The iterate
 * stays on the device between iterations, vertex-major (row 3 v + d, the frames contiguous, padded to 64), the layout the
 * projection kernels read.  No self-collisions.  Positional constraints: asb_pins_set and asb_pdsolve_pins below; external forces
 * and the floor: asb_ext_set and asb_pdsolve_external below.  One rank.  The
 * end of a time step (:531-532) is asb_pdsolve_advance below.
 * asb_pdsolve_begin: after asb_gstep_setup.  Arguments two to eleven as asb_gstep_inertia; the inertia term diag s_f is
 * formed once with that entry's arithmetic.  start 0: q_0 = s_f (the reference's), 1: q_0 = x_f, 2: q_0 = start_dev, a DEVICE
 * tensor (n_sel, n, 3).  More than 65535 * 64 selected frames: ASB_ERR_LIMIT, judged on the count alone before anything
 * else.  Drops the kinds of the previous solve and its binding of the pins; its buffers are reused. */
int asb_pdsolve_begin(asb_ctx* ctx, int which, int64_t f0, int64_t f1, int64_t fj, const double* inv_massL, int add_mean, double psf,
                      const double* diag, int mode, const double* acc3, int start, const double* start_dev);
/* Registers the kind of the preceding asb_cproj_setup as the next term of the right-hand side: its device tables pass to
 * the solve (the context has no element set-up afterwards) together with the HOST CSR of its S^T (as asb_cforce_run takes
 * and checks it), uploaded here once.  reduced != 0: the set-up holds the SAMPLED elements and the term is that of
 * asb_rforce_run with the operator and solver of the bank that is current now (asb_rforce_bank; the CSR arguments are
 * ignored): the slot records that bank.  A second reduced kind on a bank this solve has already bound is refused; reduced
 * kinds on different banks are accepted, up to the 8 slots of a solve. */
int asb_pdsolve_slot(asb_ctx* ctx, double sigma_min, double sigma_max, int reduced, int64_t n_rows, const int64_t* indptr,
                     const int64_t* indices, const double* data);
/* n_iter further iterations of the solve in progress.  chunk_frames as asb_cforce_run (no bit depends on it).  out_dev
 * (optional): caller-owned DEVICE memory (n_sel, n, 3), the iterate after the last of them, frame-major.  hist_out
 * (optional, host, n_iter x n_sel x 2): per iteration and frame [|q_new - q_old|^2, |q_new|^2] over its n x 3 entries, summed
 * in a fixed order.  The product is that of asb_gstep_run entry for entry; no atomics; repeats, sub-ranges and any chunk
 * width give identical bits.  Returns after the stream has drained. */
int asb_pdsolve_iterate(asb_ctx* ctx, int64_t n_iter, int64_t chunk_frames, double* out_dev, double* hist_out);
/* Hyper-reduced iterations: with every kind reduced (one operator per bank: one reduced kind per bank of asb_rforce_bank) an
 * iteration is q_{k+1} = c + sum_k G_{k,d} coef_{k,d}(q_k) per coordinate, c = A^-1 ms, G_{k,d} = A^-1 (S_k^T V_{k,d}), and coef
 * reads q_k only at the vertices of the sampled elements (the touched vertices): no N^2 product is left in the loop.
 * asb_hyper_operator: after asb_gstep_setup and asb_rforce_operator.  Forms G_d^T of the current bank in the layout of the
 * operator S^T V, every entry one accumulator over ascending n, and keeps it with the bank.  A later asb_gstep_setup or
 * asb_gslab_setup invalidates the G of ALL banks, a later asb_rforce_operator that of its own bank only: asb_hyper_iterate
 * then refuses (ASB_ERR_ARG) instead of using a stale operator.
 * asb_hyper_iterate: in place of asb_pdsolve_iterate, after asb_pdsolve_begin and one or more asb_pdsolve_slot, ALL with
 * reduced != 0 (a slot that is not reduced is refused), each bank with a solver and a valid G.  touched (host, n_touched,
 * strictly ascending vertices) != NULL: ONE list, the union over the kinds; the element set-up of every slot is numbered in
 * 0 .. n_touched - 1 (position in touched); iterations 1 .. n_iter - 1 run on those rows only, the last on all n rows.
 * touched NULL: the set-ups are numbered in the mesh's vertices and every iteration runs on all rows.  The two give
 * identical bits, as do repeats, sub-ranges and any chunk_frames (> 0: at most that many frames, rounded up to 64, per
 * pass; one width serves all slots, the smallest of the banks').  Within an iteration and chunk the coefficients of ALL slots
 * are formed from the old iterate before one launch writes the new one: a Jacobi update over the kinds, as the reference's.
 * out_dev (optional): caller-owned DEVICE memory (n_sel, n, 3), the iterate after the last iteration.  The whole
 * iterate is left in the solve's state.  No atomics.  Returns after the stream has drained. */
int asb_hyper_operator(asb_ctx* ctx);
int asb_hyper_iterate(asb_ctx* ctx, int64_t n_iter, int64_t n_touched, const int64_t* touched, int64_t chunk_frames, double* out_dev);

/* ------------------------------------------------ projective dynamics: time steps on the solve's state ----------- */
/* The last two lines of the reference's step (Simulators.py:531-532, :741-742: velocities = (q - positions) / dt, positions = q)
 * and the explicit state of the next step (:495), as one device operation on the state of the solve in progress.
 * asb_pdsolve_carry: after asb_pdsolve_begin.  Gives the solve P, the positions at the START of the current time step, laid
 * out like the iterate.  pos_dev NULL: P = x_f of the begun frames in world space (directly after asb_pdsolve_begin: the
 * tensor it read must still be the one on the device); otherwise a caller-owned DEVICE tensor (n_sel, n, 3).  The solve
 * keeps its own device copy of the diag that asb_pdsolve_begin was given, so a later asb_gstep_inertia does not disturb
 * it.  A new asb_pdsolve_begin drops the carry.  Returns after the stream has drained.
 * asb_pdsolve_advance: after asb_pdsolve_carry (ASB_ERR_ARG otherwise, nothing launched).  With q the iterate, per entry
 * s = fl(fl(2 q - P) + acc[d]); then P = q, the iterate = s and the inertia term = fl(diag s): the arithmetic of
 * asb_pdsolve_begin(mode 1, start 0), so an advance from (x_f, x_{f-1}) leaves its bits.  One pass, no atomics, no host
 * copy; in stream order, the call does not wait.  A time step is asb_pdsolve_iterate or asb_hyper_iterate, then this.
 * asb_pdsolve_positions: P, frame-major, into caller-owned DEVICE memory (n_sel, n, 3).  Returns after the stream has drained. */
int asb_pdsolve_carry(asb_ctx* ctx, const double* pos_dev);
int asb_pdsolve_advance(asb_ctx* ctx);
int asb_pdsolve_positions(asb_ctx* ctx, double* out_dev);
/* test hook: the iterate (which 0) or P (1) as stored, (rows = 3 n, ld = n_sel rounded up to 64) with its padding, to the host */
int asb_test_pdsolve_state(asb_ctx* ctx, int which, double* out_host, int64_t rows, int64_t ld);

/* ------------------------------------------------ projective dynamics: positional constraints (pins) ----------- */
/* PositionalConstraint of the reference (Constraint_projections.py:77-113), the first summand of b (Simulators.py:401-413,
 * :513-520): pin i holds vertex verts[i] at p0[i] + shift[row] with weight wi[i].  The weight on A's diagonal is the host's
 * business (the matrix of asb_gstep_setup / asb_gslab_setup); here the constant wi (p0 + shift[row]) of the right-hand side.
 * Pins are no kind: they take no slot and do not depend on q.
 * asb_pins_set: host arrays verts (P) in [0, n) of the tensor on the device, no two equal; wi (P) finite, >= 0; p0 (P, 3) finite;
 * shift NULL with T_s = 0 (fixed pins) or finite, (T_s, 3) (per_pin 0) or (T_s, P, 3) (per_pin != 0).  Checked, then uploaded once
 * into buffers the context owns; replaces the previous pins and drops their binding to a solve.  Any violation: ASB_ERR_ARG,
 * no pins are left.  asb_pins_clear: no pins, no binding (the buffers stay for the next set).
 * Arithmetic, everywhere: t = fl(p0 + shift[row]) (p0 without a shift), term = fl(wi t) rounded on its own, then the add.
 * asb_pins_term: the term of the frames range(f0, f1, fj), frame f with row row0 + f, into the caller's DEVICE tensor
 * (n_sel, n, 3).  accumulate 0: every entry is written, +0.0 where a vertex is not pinned; != 0: out = fl(out + term) at the
 * pinned entries, nothing else touched.  A row outside shift: ASB_ERR_ARG, nothing launched.  One thread per (frame, pin), no
 * atomics.  Returns after the stream has drained.
 * asb_fm_add: a = fl(a + b) entry by entry on two caller-owned DEVICE tensors of len doubles that do not overlap: the add of an
 * iteration (b += ms), for a caller that forms fl(sum of the kinds + fl(fl(diag s) + pin term)) as a solve does.
 * asb_pdsolve_pins: after asb_pdsolve_begin (ASB_ERR_ARG before, or a second time).  Binds the context's pins to the solve in
 * progress and adds their term to the inertia term: frame f reads row row0 + f.  From then on asb_pdsolve_advance launches the
 * same kernel behind its own with the row raised by one per advance; an advance (or this call) that would read a row >= T_s
 * returns ASB_ERR_ARG and launches nothing.  asb_pdsolve_iterate, asb_hyper_iterate and the slab path read the inertia term
 * and are not changed.  In stream order; the call does not wait. */
int asb_pins_set(asb_ctx* ctx, int64_t P, const int64_t* verts, const double* wi, const double* p0, int64_t T_s, const double* shift,
                 int per_pin);
int asb_pins_clear(asb_ctx* ctx);
int asb_pins_term(asb_ctx* ctx, int64_t f0, int64_t f1, int64_t fj, int64_t row0, int accumulate, double* out_dev);
int asb_fm_add(asb_ctx* ctx, double* a_dev, const double* b_dev, int64_t len);
int asb_pdsolve_pins(asb_ctx* ctx, int64_t row0);

/* ------------------------------------------------ projective dynamics: external forces and the floor ----------- */
/* The start of the reference's step (Simulators.py:494-498): explicit = positions + dt velocities + dt^2 fext / mass, then
 * resolve_collision (Constraint_projections.py:1287-1298) on every vertex of it -- a coordinate below the floor is set onto it --,
 * and both the inertia term and the first iterate are taken from the result.  Gravity stays in acc3 of asb_pdsolve_begin; the
 * table holds fa = dt^2 force / mass of the remaining forces, formed by the host.  Arithmetic, per entry (row 3 v + d, frame
 * column c, table row rho(c) = row0 + f0 + c fj + step), after s = fl(fl(2 q - P) + acc[d]) of asb_pdsolve_advance (or the s
 * of asb_pdsolve_begin):  x = fl(s + fa[rho(c)][3 v + d]);  if (d == axis && x < height) x = height;  iterate = x,
 * inertia term = fl(diag[v] x).  The add is rounded on its own; the floor is a comparison, so NaN stays NaN in its frame.
 * asb_ext_set: table_host (T_s, 3 n) finite doubles with T_s > 0, one row per step; (3 n) with T_s = 0, a constant force; NULL:
 * no forces (floor only).  floor_on != 0: the floor along axis (0..2) at the finite height.  Checked against the n vertices of
 * the tensor on the device, then uploaded once into a buffer the context owns; replaces the previous forces and floor and drops
 * their binding to a solve.  A table of more than 2^31 bytes: ASB_ERR_LIMIT; any other violation, or neither a table nor a
 * floor: ASB_ERR_ARG; nothing is left set.  asb_ext_clear: nothing set, no binding (the buffer stays for the next set).
 * asb_pdsolve_external: after asb_pdsolve_begin (and asb_pdsolve_carry, and the asb_pdsolve_advance of a continuation), BEFORE
 * asb_pdsolve_pins -- this call rewrites the inertia term, so with the pins bound it is refused, as it is before a begin, a
 * second time, with nothing set, and with forces checked against another n.  Checks the rows step 0 needs (a missing row:
 * ASB_ERR_ARG, nothing launched), binds, and corrects the state in one pass: the iterate holds s, the two lines above are
 * applied to it and the inertia term is rewritten.  With start 1 or 2 of asb_pdsolve_begin the iterate is not s: s is then
 * formed as start 0 forms it into a scratch tensor, only the inertia term is rewritten and the iterate is left alone.  From
 * then on asb_pdsolve_advance first checks the next step's row (missing: ASB_ERR_ARG, nothing launched, the state untouched)
 * and runs its pass with the two lines fused in, one row further per advance: T1 steps continued by T2 (row0 raised by T1)
 * equal T1 + T2 steps bit for bit.  A new asb_pdsolve_begin drops the binding.  Returns after the stream has drained. */
int asb_ext_set(asb_ctx* ctx, int64_t T_s, const double* table_host, int floor_on, int axis, double height);
int asb_ext_clear(asb_ctx* ctx);
int asb_pdsolve_external(asb_ctx* ctx, int64_t row0);

/* ------------------------------------------------ SPLOCS refinement ----------- */
/* posComponents.splocs_glob_optimization, snapbases/posComponents.py:132-189.
 * State after a residual-mode deflation: C = comps, W = weigs, U = 0 (:135-139).  One outer
 * iteration = weights -> (host support maps) -> admm -> gram -> objective.  The F x 3N
 * residual is never formed (see csrc/asb_splocs.hip).  No limit on K of its own: K <= 64 runs the ADMM loop in one fused
 * launch, larger K the unfused loop (tested up to K = 136); the weight sweep spreads over blocks while 64 rows of W fit the
 * LDS (K <= 298) and runs in one block beyond. */
int asb_splocs_begin(asb_ctx* ctx);
/* P = X C^T (F x K) and M = C C^T (K x K) of this shard for the CURRENT C, into the
 * caller's device buffers (to be all-reduced over ranks) or into the context when NULL.
 * normX2_local (optional): |X|^2 of the shard. */
int asb_splocs_gram(asb_ctx* ctx, double* P_dev, double* M_dev, double* normX2_local);
/* :144-156 weight sweep with the (all-reduced) P, M (NULL: the context's own), G = W^T W;
 * centre_idx/val (K): per component this shard's vertex of largest |C_k[v]|^2 (:161). */
int asb_splocs_weights(asb_ctx* ctx, const double* P_dev, const double* M_dev,
                       int64_t* centre_idx, double* centre_val);
/* :167-181 ADMM with Lambda (host, K x n_loc) = splocs_lambda * support_map; C = Z at the end */
int asb_splocs_admm(asb_ctx* ctx, const double* Lambda, double rho, int n_iter);
/* the same step with Lambda built on the device: Lambda[k] = lambda * (clip(phi_k, dmin, dmax) - dmin) / (dmax - dmin)
 * (:162-165, utils/support.py:61-64) from the cached distance field in slot slots[k] (K slots, host) */
int asb_splocs_admm_fields(asb_ctx* ctx, const int64_t* slots, double lambda, double dmin, double dmax, double rho, int n_iter);
/* :183-186 pieces of the objective for the new C (call asb_splocs_gram first):
 * wp = <W, P>, gm = <W^T W, M>  =>  |X - W C|^2 = |X|^2 - 2 wp + gm;
 * sparsity_local = sum Lambda |C_v| over the shard. */
int asb_splocs_objective(asb_ctx* ctx, const double* P_dev, const double* M_dev, double* wp,
                         double* gm, double* sparsity_local);
/* refined components (K, n_loc, 3) and weights (F, K); either may be NULL */
int asb_splocs_results(asb_ctx* ctx, double* C_out, double* W_out);

/* ------------------------------------------------ host-side probes ----------- */
/* the small dense solvers of csrc/asb_smalldense.hip on host arrays (tests):
 * tridiagonal (d, e) -> all eigenvalues descending + k leading unit eigenvectors Z (n x k row-major);
 * one-sided Jacobi on the rows of A (nv x m): singular values descending, left vectors as COLUMNS of U (nv x nv, optional);
 * Tt[c][i] = (L^-1)[i][c] of the Cholesky factor G = L L^T (any K). */
int asb_test_tridiag_eig(asb_ctx* ctx, const double* d, const double* e, int64_t n, int64_t k, double* lam_desc, double* Z,
                         int64_t* n_bad);
int asb_test_jacobi_rows(asb_ctx* ctx, const double* A, int64_t nv, int64_t m, double* U, double* sig, int64_t* sweeps);
int asb_test_chol_tinv(asb_ctx* ctx, const double* G, int64_t K, double* Tt);
/* The 3x3 symmetric eigen-solver used by asb_deflate_pick, run on the HOST (unit test
 * without a GPU).  a6 = (a00,a01,a02,a11,a12,a22); out4 = (lambda_max, u0, u1, u2). */
void asb_test_eig3(const double* a6, double* out4);
/* test hooks of the greedy step (csrc/asb_kernels.h; tests/test_deflate_step_cpu.py, tests/test_gpu_deflate_step.py).
 * asb_test_eig3_fast: as asb_test_eig3 for the root-and-cross-product solver of the panel kernel and the sketch replay (host).
 * asb_test_pick_cfg: the stream configuration of a padded row length Fp on the host: out5 = (ok, T, E2, block, vpb).
 * asb_test_eig3_dev: either solver (fast = 0 / 1) on the device, one thread per matrix: a6 (n x 6) -> out4 (n x 4); all of out4
 * (out_len >= 4 n doubles) round-trips, so a write behind the result shows.
 * asb_test_deflate_step: residual mode; installs w (F doubles, the row's padding zeroed) and |w|^2 = wn2 as component k and runs
 * asb_deflate_apply(k, s) on them.
 * asb_test_deflate_state: what the context holds, every pointer optional: energy (n_loc), the partial records of the last streaming
 * pass pmax / pidx / psum (counts[0] of them; room for counts[1] = the grid cap), scal ((K + 1) x 4: sigma, |w|^2, index bits, local
 * |R|^2), W (K x Fp) and R (3 n_loc x Fp) with their padding.
 * asb_test_local_best: asb_deflate_local_best(k) into the context's record, copied to rec (asb_deflate_xchg_len doubles).
 * asb_test_pick_records: asb_deflate_pick(k) over n_rec (<= 16) records given on the host. */
void asb_test_eig3_fast(const double* a6, double* out4);
void asb_test_pick_cfg(int64_t Fp, int* out5);
int asb_test_eig3_dev(asb_ctx* ctx, int fast, const double* a6, int64_t n, double* out4, int64_t out_len);
int asb_test_deflate_step(asb_ctx* ctx, int64_t k, const double* w, double wn2, const double* s);
int asb_test_deflate_state(asb_ctx* ctx, double* energy, double* pmax, int64_t* pidx, double* psum, int64_t* counts, double* scal,
                           double* W, double* R);
int asb_test_local_best(asb_ctx* ctx, int64_t k, double* rec);
int asb_test_pick_records(asb_ctx* ctx, int64_t k, const double* recs, int64_t n_rec);
/* The 3x3 rotation solve of asb_align_frames (procrustes_rot, csrc/asb_kernels.h), run on the HOST: m9 = the cross-covariance M
 * row-major, out9 = R row-major (tests/test_procrustes_rot_cpu.py). */
void asb_test_procrustes_rot(const double* m9, double* out9);
/* "Project F" of the constraint projections (cp_project_tri / cp_project_tet, csrc/asb_cproj_elem.h) on its own: n stored
 * deformation gradients, row-major -- kind 1 (tris_strain) 2 x 2 -> Fhat 2 x 2; kind 2 (tets_strain) 3 x 3 -> U diag(c) V^T;
 * kind 3 (tets_deformation_gradient) 3 x 3 -> R^T, as the kernels store it -- with the clamp [sigma_min, sigma_max].
 * asb_test_cproj_project runs on the HOST; asb_test_cproj_project_dev on the device, one thread per matrix, no context state;
 * all of out (out_len >= n x the kind's width) round-trips, so a write behind the result shows
 * (tests/test_cproj_model_cpu.py, tests/test_gpu_cproj_edges.py). */
int asb_test_cproj_project(int kind, const double* mats, int64_t n, double sigma_min, double sigma_max, double* out);
int asb_test_cproj_project_dev(asb_ctx* ctx, int kind, const double* mats, int64_t n, double sigma_min, double sigma_max, double* out,
                               int64_t out_len);
/* tests: the sketch replay on host arrays -- cols (r x 3 n: column i, entry 3 v + d, the coefficient of vertex v's row d on the
 * unit direction i divided by sqrt(wn2[i])), wn2 (r), exact energies E (n) -> scores (n; max over the steps of energy / winner's
 * energy), the replay's winners pred (steps; -1 behind its end), *status = 1 (0: the exchange timed out, scores = energies) */
int asb_test_sketch_predict(asb_ctx* ctx, const double* cols, const double* wn2, const double* E, int64_t n, int r, int steps,
                            double* scores, int64_t* pred, int* status);
/* test hook: inverse of a host symmetric positive definite matrix (n x n) through the device's blocked
 * Gauss-Jordan / f64-MFMA GEMM path that the device geodesics use for their two SPD systems */
int asb_test_spd_inverse(asb_ctx* ctx, const double* A_host, int64_t n, double* Ainv_host);
/* test hook: out (out_cols x 3 n_loc, host, in and out) gets, in columns j < ncols, X . W[:, k0 + j] / col_scale[k0 + j] -- X the
 * uploaded snapshots (row 3 v + d of the shard), W (F x ldw, host, frame-major), col_scale (ldw, host; NULL: 1).  All of `out`
 * travels to the device and back, so a write beyond the ncols columns shows.  path 0: the 16-column kernel, one pass per 16
 * columns; path 1: the multi-tile kernels in one pass (ceil(ncols / 16) tiles, ncols <= 128; ASB_WIDE_VARIANT applies). */
int asb_test_project_columns(asb_ctx* ctx, const double* W_host, int64_t ldw, int64_t k0, int ncols, const double* col_scale_host,
                             int path, double* out_host, int64_t out_cols);
/* test hooks of the dense f64 building blocks on host arrays.  Operands travel whole (with NaN behind them), outputs round-trip
 * whole, so a write outside the result shows; arguments are refused as the wrapped function refuses them.
 * asb_test_gemm_nn: C (c_len doubles, ld ldc) = beta C + alpha A B through asb_gemm_nn (split-K, the triangular form `tri` and the
 * C -= A B form chosen by its own rules); A (M x lda), B (Kc x ldb).
 * asb_test_gemm_tn: X (R x ldx), Y (R x ldy), out (out_len doubles).  form 0: out[i so_i + j so_j] = sum_r X[r ldx + i sx] Y[r ldy + j]
 * (the one-wave-per-tile kernel, contraction split as for an I_split-row product when I_split > 0); form 1: out (I x J) = X^T Y on
 * the 128 x 128-tile kernel; form 2: out (I x I) = X^T X on its symmetric form (J = I, Y unused).
 * asb_test_transpose: out[c rows + r] = in[r cols + c] (out_len >= rows cols).
 * asb_test_sym_eig: the one-block Jacobi solver (n <= 128): lam descending, V (n x n) eigenvectors as columns, *status = its
 * status word (2: no convergence). */
int asb_test_gemm_nn(asb_ctx* ctx, const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int64_t M,
                     int64_t N, int64_t Kc, double alpha, double beta, int tri, int64_t c_len);
int asb_test_gemm_tn(asb_ctx* ctx, int form, const double* X, int64_t ldx, int64_t sx, const double* Y, int64_t ldy, int64_t R,
                     int64_t I, int64_t J, double* out, int64_t so_i, int64_t so_j, int64_t out_len, int64_t I_split);
int asb_test_transpose(asb_ctx* ctx, const double* in, int64_t rows, int64_t cols, double* out, int64_t out_len);
int asb_test_sym_eig(asb_ctx* ctx, const double* A, int64_t n, double* lam, double* V, int* status);
/* test hooks of the SPLOCS phases (tests/test_gpu_splocs_phases.py), after asb_splocs_begin; host arrays, every pointer optional.
 * asb_test_splocs_install: overwrites the state: C (K, n_loc, 3), W (F, K) frame-major, U (K, n_loc, 3).
 * asb_test_splocs_state: what the last phase left: U (K, n_loc, 3), Lambda (K, n_loc), G = W^T W and Ginv = (G + rho I)^-1 (K, K),
 * c = W^T X (K, 3 n_loc).  G is written by asb_splocs_weights, the others by asb_splocs_admm(_fields). */
int asb_test_splocs_install(asb_ctx* ctx, const double* C, const double* W, const double* U);
int asb_test_splocs_state(asb_ctx* ctx, double* U, double* Lambda, double* G, double* Ginv, double* c);
/* test hooks of the device geodesics (tests/test_gpu_geodesic_small.py); host arrays, no solver state is changed.
 * asb_test_slab_gemm64: out (M x 64, in and out) = beta out + alpha A (M x lda, Kc columns used) Z (Kc x 64) on the slab sweeps'
 * product kernel with nct (clamped to 1 .. 4) column tiles of 16: columns >= 16 nct stay as they are.  M, Kc multiples of 16.
 * asb_test_geodesic_field1: phi_out (n) = the field asb_deflate_apply_geodesic solves for its source, for a source given here
 * (dense mode: the single-source path; otherwise the batch solver with one source).
 * asb_test_support_weights: s_out (n_loc) = 1 - (clip(phi[v0 + i], dmin, dmax) - dmin) / (dmax - dmin) on the device, phi (n) host.
 * asb_test_geodesic_cached: out (n) = the cached field of `slot`; ASB_ERR_ARG where there is none. */
int asb_test_slab_gemm64(asb_ctx* ctx, const double* A, int64_t lda, const double* Z, double* out, int64_t M, int64_t Kc,
                         double alpha, double beta, int nct);
int asb_test_geodesic_field1(asb_ctx* ctx, int64_t src, double* phi_out);
int asb_test_support_weights(asb_ctx* ctx, const double* phi, int64_t n, int64_t v0, int64_t n_loc, double dmin, double dmax,
                             double* s_out);
int asb_test_geodesic_cached(asb_ctx* ctx, int64_t slot, double* out);
/* test hook of the snapshot preparation (tests/test_gpu_prep.py): what the context holds, every pointer optional.  X_raw: the
 * vertex-major tensor (3 n_loc x Fp) WITH its padding; E0, EV (n_loc each): the per-vertex energies of the last scaling sweep;
 * scalars10: the six device scalars [|X|^2, largest E0, energy along the constant-in-time direction, -, sum EV, sum EV^2]
 * followed by the host fields ev_cv2, mean_frac, mean_energy, prep_normx2; flags3: e0_valid, ev_valid, have_mean.
 * The energies, scalars and host fields are whatever the last scaling sweep on this context left: they describe the CURRENT
 * tensor only while e0_valid / ev_valid are set (a later writer of X clears the flags and leaves the arrays as they are).
 * ASB_ERR_ARG with a message where a buffer that was asked for does not exist (no ingest call / no scaling sweep yet). */
int asb_test_prep_state(asb_ctx* ctx, double* X_raw, double* E0, double* EV, double* scalars10, int* flags3);

#ifdef __cplusplus
}
#endif
#endif /* ASB_H */
