// Internal definitions shared by the translation units of libasb_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "asb.h"

// Device-resident state of one panel of the projection path (asb_project.hip).
#define ASB_PANEL_COLS 16          // steps (weight columns) per panel = columns of one projection pass

struct PanelState {
    double theta;          // upper bound on the energy of every NON-candidate vertex
    double margin;         // absolute safety margin on that bound (rounding of the energy recurrence)
    long long done;        // set when the best candidate can no longer be proven to be the global arg-max
    long long committed;   // components committed in this panel
    long long n_cand;
    long long pad;
    // steps taken without proof (verified against every vertex's energy after the projection pass, k_correct<true>)
    long long proven;      // length of the provable head of the panel (-1 until the panel kernel has set it)
    long long spec_max;    // how many unproven steps the panel kernel may add
    long long spec_ok;     // first unproven step the verification rejected (>= committed: none)
    double e_win[16];      // energy of each step's winner
};

struct StreamCfg {
    int T, E2, block, vpb;
};

struct asb_splocs;
struct asb_geo;
struct asb_pds;
struct asb_gsl;
struct asb_gsb;
struct asb_zr;

// world positions of the resident tensor (asb_cproj.hip): x = (T * inv_psf + mean) * invm_v
struct CpWorld {
    const double* T;
    long long ldt;
    const double* mean;
    const double* invm;
    double inv_psf;
};
#ifdef __HIPCC__
__device__ __forceinline__ void cp_pos(const CpWorld& w, long long f, int v, double (&x)[3]) {
    const double im = w.invm ? w.invm[v] : 1.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) x[d] = (w.T[(3LL * v + d) * w.ldt + f] * w.inv_psf + (w.mean ? w.mean[3LL * v + d] : 0.0)) * im;
}
#endif

// One element set-up on the device: what asb_cproj_setup uploads.  The context holds one (ctx->cp: the kind of the next
// asb_cproj_run / asb_cforce_run / asb_rforce_run) and every slot of a solve holds one (asb_pdsolve.hip), taken over from the
// context by asb_cp_move.
struct CpSetup {
    int kind = -1;                    // element kind (-1: no set-up)
    int64_t n = 0, verts = 0;         // its elements; the vertices its indices were checked against
    int64_t vmax = -1;                // largest vertex it names (elements and star edges)
    int *idx = nullptr, *sptr = nullptr, *sidx = nullptr;    // indices (n x width); verts_bending: star CSR
    double* table = nullptr;          // per-element tables (n x TW), verts_bending: followed by the star edges' weights
};

struct asb_ctx {
    int dev = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    std::map<void*, size_t> alloc_bytes;   // capacity of each context-owned buffer

    // ---- snapshot shard, vertex-major: row r = 3*v + d, Fp doubles per row ----
    int64_t F = 0, Fp = 0, n_loc = 0, v0 = 0, N_glob = 0;
    // X is a VIEW, never an asb_alloc key: of X_in (what the last ingest call wrote) or, between
    // asb_pod_deflate_begin and _end, of X_lvl (the level's deflated copy)
    double *X = nullptr, *X_in = nullptr, *X_lvl = nullptr;   // (3*n_loc, Fp) prepared snapshots (snapTensor)
    double* mean = nullptr;   // (3*n_loc)
    bool have_mean = false;
    // per-vertex energies |X_v|^2 of the PREPARED tensor, a by-product of the last sweep that wrote it (k_scale_energy) or
    // of the first projection-mode begin after X changed; every writer of X clears e0_valid
    double* tr_part = nullptr;  // per-strip [sum, sum of squares] of the fused layout change
    double* E0 = nullptr;       // (n_loc)
    double* e0_sc = nullptr;    // [|X|^2 of the shard, largest energy, energy along the constant-in-time direction]
    // EV[v] = E0[v] - sum_d (sum_f X[v,d,f])^2 / F: the energy left once the constant-in-time direction is gone -- what the
    // first panel uses to GUESS its later winners when that direction carries much of |X|^2 (mean_frac; rest shape "first")
    double* EV = nullptr;
    int* hist6 = nullptr;             // histograms / range blocks of the scores of a guessed selection
    double* scm = nullptr;
    bool hist6_clear = false;
    double* mean_part = nullptr;      // per-block partials of that energy
    double ev_cv2 = 0.0;            // squared coefficient of variation of EV over the vertices (asb_snapshots_scale)
    double mean_frac = 0.0, mean_energy = 0.0, prep_normx2 = 0.0;     // share / energy along that direction, |X|^2 (host)
    int64_t m_target_eff = 0;   // != 0 while a guessed panel is being selected: the (smaller) target of the energies proper
    int first_panel_mean = 1;   // ASB_FIRST_PANEL_MEAN=0: first panel from the initial energies alone
    const double* sel_e2 = nullptr;      // != NULL while a panel's candidates are { E > tau } u { sel_e2 > tau_v }
    bool e0_valid = false;
    bool ev_valid = false;          // EV / mean_energy / prep_normx2 describe the CURRENT tensor (set by asb_snapshots_scale only; every
                                    // writer of X and asb_project_begin's own energy pass clear it)
    int64_t n_energy_pass = 0;  // reads of X the last asb_deflate_begin spent on initial energies (statistics)

    // ---- reduction scratch ----
    int nblk_cap = 0;
    double* pmax = nullptr;
    long long* pidx = nullptr;
    double* psum = nullptr;
    double* scalar_dev = nullptr;   // a few doubles for device-side scalars
    double* s_dev = nullptr;        // (n_loc) support factor

    // ---- deflation state ----
    int64_t K = 0;
    int mode = 0, local = 0;
    int64_t k_done = 0;
    // overlapped download of the basis (asb_components_stream): pinned (K, n_loc, 3) buffer, copy stream, rows enqueued so far
    int dl_enabled = 0;
    double* dl_host = nullptr;
    size_t dl_host_count = 0;
    int dl_host_owned = 1;            // 0: the caller's buffer (asb_components_stream_into): never freed here
    hipStream_t dl_stream = nullptr;
    hipEvent_t dl_event = nullptr;
    long long dl_done = 0;
    double* res_pin = nullptr;        // pinned host slot of a run's small results (asb_project_results): [seq, -, (K+1) x 4 scalars, 8 range scalars]
    double* res_pin_dev = nullptr;
    size_t res_pin_count = 0;
    double* td_wy = nullptr;          // blocked back-transformation: T factors, reflector panels, work
    // the sparse differential operator S^T of the constraint path (asb_st_upload: CSR on the device) and its work arrays
    long long* st_indptr = nullptr;
    long long* st_indices = nullptr;
    double* st_data = nullptr;
    long long st_rows = 0, st_cols = 0, st_nnz = 0;
    double* st_energy = nullptr;      // (st_rows) squared row norms of S^T M
    double* st_amax = nullptr;        // (st_rows) largest |entry| per row of S^T M
    double* st_resid = nullptr;       // (n_loc, 3 p) residual block of the position-space interpolation error
    // several ranks (asb_st_upload_shard, asb_pod.hip): the S^T rows of the position vertices this rank owns, columns remapped
    // to local slots -- [0, n_loc) this shard, [n_loc, n_loc + st_h) the halo -- and the halo copies of residual / basis rows
    long long* sh_indptr = nullptr;
    long long* sh_indices = nullptr;
    double* sh_data = nullptr;
    long long sh_rows = 0, sh_nnz = 0, st_h = 0, sh_n_loc = -1;
    double* sh_energy = nullptr;      // (sh_rows) squared row norms of S^T M over the owned vertices
    double* sh_amax = nullptr;        // (sh_rows) largest |entry| per owned row
    double* halo_R = nullptr;         // (st_h, 3 Fp) residual rows, deflated with every component like the owner's
    double* halo_C = nullptr;         // (halo_K, st_h, 3) basis rows
    long long halo_K = 0;             // K of the filled halo basis (0: none)
    int halo_R_ok = 0;                // the halo residual was filled for the current upload
    double* halo_energy = nullptr;    // k_stream scratch of the halo pass: (st_h) energies, (st_h, 3) coefficients, partials
    double* halo_ck = nullptr;
    double* halo_pmax = nullptr;
    long long* halo_pidx = nullptr;
    double* halo_psum = nullptr;
    double* halo_resid = nullptr;     // (st_h, 3 p) residual block of the position-space interpolation error on the halo
    long long* halo_map = nullptr;    // pack / fill row lists
    unsigned* coop_bar = nullptr;     // k_panel_multi: flags [-, abort, too many candidates, -] + debug timestamps
    double* coop_rec = nullptr;       // (2, grid) records {e, lam, wn2, slot}
    int panel_coop = 1;               // ASB_PANEL_COOP=0 -> the two-kernel inner loop
    int e0_reuse = 1;                 // ASB_E0_REUSE=0 -> asb_project_begin always re-reads X for the initial energies
    int correct_rows = 1;             // ASB_CORRECT_ROWS=0 -> the one-thread-per-vertex correction kernel (k_correct)
    int coop_test_stall = 0;          // ASB_COOP_TEST_STALL=1 (tests): the first co-resident launch is made to time out
    int64_t n_guess_panels = 0;       // first panels of the last run whose candidates were guessed (asb_project_run)
    int64_t n_coop_fallbacks = 0;     // launches of k_panel_coop whose record exchange timed out (redone by the two-kernel loop)
    int64_t n_coop_launches = 0;      // launches of the co-resident panel kernel (k_panel_multi) in the last run
    int64_t max_read_kept = 0;        // most components one read of X (all its sub-panels) committed in the last run
    int spec_panels = 1;              // ASB_SPEC_PANELS=0 -> provable steps only
    int spec_budget = 16;             // adapted to how many unproven steps survived in the last panels
    // joins asb_panel_project_spec[_dev] to the asb_panel_commit that follows it: the provable head of the panel being checked
    long long spec_proven = 0;
    double* w_fk = nullptr;                 // weights in the reference's (F, K) order for the read-back
    unsigned char* host_pin = nullptr;      // pinned (coherent, device-mapped) host memory for the small read-backs
    unsigned char* host_pin_dev = nullptr;  // its device address: tiny kernels publish state there, the host polls (asb_pin_alloc)
    unsigned long long pin_seq = 0;         // sequence number of the last publication
    long long n_spec_steps = 0, n_spec_kept = 0;      // statistics (asb_deflate_stats)
    double *Wt3 = nullptr, *wn2t3 = nullptr, *Wq3 = nullptr, *gram3 = nullptr;
    int64_t forced_row = -1;      // asb_deflate_force_next: global row the next pick must take
    double* bam_val = nullptr;    // asb_deflate_block_argmax partials
    long long* bam_idx = nullptr;
    int nblk = 0;               // partial records written by the last streaming pass
    double* R = nullptr;        // (3*n_loc, Fp) residual (mode RESIDUAL)
    double* energy = nullptr;   // (n_loc)
    double* W = nullptr;        // (K, Fp)
    double* comps = nullptr;    // (K, 3*n_loc)
    double* scal = nullptr;     // (K+1, 4): sigma, |w|^2, idx bits, local ||R||^2 after comp k
    double* xrec = nullptr;     // one exchange record

    // ---- projection (panel) path, asb_project.hip ----
    int n_cu = 256;
    StreamCfg cfg{};
    int64_t m_target = 0, m_cap = 0;   // candidate-set size aimed for / capacity
    double* Wt = nullptr;        // (Fp, 16) panel weights, frame-major (MFMA B operand order)
    double* wn2t = nullptr;      // (16) |w_t|^2 of the panel
    double* candR = nullptr;     // (m_cap, 3, Fp) exact residual rows of the candidates
    double* cand_e = nullptr;    // (m_cap)
    double* cand_c = nullptr;    // (16, m_cap, 3) in-panel coefficients of the candidates
    double* slab_scratch = nullptr;
    long long* cand_idx = nullptr;
    double* cpmax = nullptr;     // partial records of passes over the candidate buffer
    long long* cpidx = nullptr;
    double* cpsum = nullptr;
    int cnblk = 0;
    int64_t n_slots_host = 0;   // candidates in the assembled (multi-rank) buffer
    double* colpart = nullptr;   // (blocks, 16)
    double* gram = nullptr;      // (K, 16) w_j . w_panel
    double* gram_s = nullptr;    // the same divided by |w_t|^2 of the panel's column t (k_correct_rows)
    double* ypart = nullptr;     // partial 16x16 tiles between sweeps of k_project_lds
    unsigned int* tile_counter = nullptr;
    double* Wq = nullptr;        // (Fp/16, 4, 16, 4) panel in MFMA lane order (k_project_l2)
    long long* ctmp = nullptr;   // compaction scratch
    long long* ccnt = nullptr;
    int* hist = nullptr;
    PanelState* pstate = nullptr;
    PanelState* pstate2 = nullptr;         // double panels: the first sub-panel's state, kept for its check after the pass
    int double_panels = 1;                 // two sub-panels per read of X (ASB_DOUBLE_PANELS=0: one)
    double* e_class = nullptr;             // energies at the start of a double panel: who was a candidate (both tiles' checks)
    double* e_tmp = nullptr;               // energies as if a tile stood in full (k_correct_rows<true> -> k_apply_tmp)
    double* wide_out = nullptr;            // asb_project_columns_wide: where the multi-tile pass writes (default: comps)
    double* e_tmp4 = nullptr;              // k_check_tiles_w: tentative energies per tile (4 x n_loc)
    double* chk_rec = nullptr;             // its per-tile block records: pmax | psum | colpart (4 x nblk_cap x (1 + 1 + 16))
    long long* chk_idx = nullptr;
    long long* tile_res = nullptr;         // per tile: columns kept (-1: not reached); [ASB_MAX_SUB]: the chain flag
    int sub_chain = 1;                     // the sub-panels of a read enqueued without host reads in between (ASB_SUB_CHAIN=0: one by one)
    int tile_chain = 1;                    // tiles of a read finished without host reads in between (ASB_TILE_CHAIN=0: one read per tile)
    int pre_orth = 1;                      // multi-sub-panel reads project on pre-orthogonalised weights (ASB_PRE_ORTH=0: correct after)
    int sub_panels = 4;                    // most sub-panels per read of X with double_panels (ASB_SUB_PANELS, 1..8; from 5 on
                                           // the projection kernel needs more than 256 registers and loses what the saved read gains)
    int sub_first = 4;                     // sub-panels of the first read (ASB_SUB_FIRST); then adapted: sub_cur
    int sub_cur = 0;
    // joins asb_panel_read_run to the asb_panel_read_commit that follows it (the multi-rank driver's read in progress): its tiles,
    // the grid of its checks
    long long rd_k0 = 0;
    int rd_ntile = 0, rd_nc[8] = {0}, rd_proven[8] = {0}, rd_rgrid = 0;
    double* rd_words = nullptr;            // (8) per tile: columns that stand on this shard; [ASB_MAX_SUB]: status
    int sub_budget[8] = {16, 16, 16, 16, 16, 16, 16, 16};      // steps given to the later sub-panels (adapted to what the last ones kept)
    int64_t n_panels = 0, n_refresh = 0;
    // stall cliff: a run whose reads of X commit fewer than 3/4 of a component each (K beyond the numerical rank: nothing is
    // provable at rounding level, every panel ends in an exact refresh) continues in the residual loop (asb_project_switch_residual)
    int stall_fallback = 1;                // ASB_STALL_FALLBACK=0: keep grinding through panels
    int64_t fb_mark_reads = 0, fb_mark_k = 0;
    int64_t k_switch = -1;                 // component at which this run left the projection mode (-1: it did not)
    // sketch predictor (asb_sketch.hip): candidates of the next read named by a greedy replay in the space of the columns
    // the last read computed for its rejected steps
    int sketch = 1;                        // ASB_SKETCH=0: candidates by energy (and the first panel's guess) only
    bool sketch_valid = false;             // sk_score holds the scores for the read about to start
    bool read_by_score = false, last_by_score = false;      // the read in progress / the one before took predicted candidates
    double rate_plain = -1.0, rate_sketch = -1.0;           // components per modelled ms of the two kinds of read (exponential means)
    int mode_streak = 0, probe_after = 2;
    // measured cost (ms) of a read with 1 .. 4 sub-panels and of a 64-step replay on this context and shape (-1: not seen yet)
    double cost_nt[5] = {-1.0, -1.0, -1.0, -1.0, -1.0}, cost_replay = -1.0;
    int cost_cnt[5] = {0, 0, 0, 0, 0}, cost_replay_cnt = 0;
    int64_t cost_n = 0, cost_Fp = 0;
    bool sketch_run_off = false;           // this run's data are noise-like (a sketch held too little of the residual): no more replays
    unsigned long long* sk_words = nullptr;
    unsigned* sk_flags = nullptr;          // [-, abort, ran to the end, -]
    int* sk_map = nullptr;                 // replay subset (shards above one co-resident launch): slot -> vertex, increasing
    int* sk_cnt = nullptr;
    double* sk_score = nullptr;            // (n_loc)
    long long* sk_pred = nullptr;          // (64) the replay's winners
    unsigned* sk_counts = nullptr;         // [replays run, launches that found the sketch too thin and left score = energy]
    int sk_test_stall = 0;                 // tests: the next launch is made to time out
    int64_t n_sketch_runs = 0, n_sketch_reads = 0;
    // diversity family of a candidate selection (asb_project.hip: in_div): energy-weighted random vertices beside the largest
    int diverse = 1;                       // ASB_DIVERSE=0: candidates by energy / guess / replay scores only
    bool diverse_next = false;             // the next plain read takes half of its candidates by the weighted sample
    bool read_diverse = false;             // the read in progress does
    int64_t n_diverse_reads = 0;

    asb_splocs* splocs = nullptr;   // SPLOCS state (asb_splocs.hip)
    asb_geo* geo = nullptr;         // device geodesics (asb_geodesic.hip)
    long long* geo_src = nullptr;
    double* geo_out = nullptr;

    // ---- small dense linear algebra scratch (asb_linalg.hip) ----
    double* la_part = nullptr;
    size_t la_part_cap = 0;
    double* comps2 = nullptr;     // second basis buffer (orthogonalisation output)
    double* og = nullptr;         // (3, K, K) per-dimension Gram / scaled eigenvectors
    double* olam = nullptr;       // (3, K)
    double* oct = nullptr;        // (3 n_loc, K) transposed basis
    double* ovec = nullptr;       // (3, K, K) eigenvectors
    double* osing = nullptr;      // (3, K) singular values
    double* la_vtmp = nullptr;
    double* kk_tmp = nullptr;     // K x K transposed factor (asb_combine_rows)
    double *pod_g = nullptr, *pod_v = nullptr, *pod_s = nullptr, *pod_coef = nullptr;   // asb_pod.hip
    double* pod_vn = nullptr;     // (F x K) right Ritz vectors / sigma of the power step
    // the POD in levels (asb_pod_deflate_begin / _end): bases kept by finished levels
    double* pod_u1 = nullptr;
    int64_t pod_u1_rows = 0;
    int* la_status = nullptr;
    double* dn_sym = nullptr;                     // symmetric Gauss-Jordan: pivot row panel, D x panel, signed transpose, pivot block
    double *dn_work = nullptr, *dn_test = nullptr;   // asb_dense.hip: Gauss-Jordan panels; test matrix
    double* td_backup = nullptr;                  // the matrix before the panels (restored if a panel's exchange times out)
    double* td_panel = nullptr;                   // k_td_panel: x | z partials | V | W | p, q
    unsigned long long* td_rec = nullptr;         // its exchange words (ring of three) and the abort flag
    double* td_ppart = nullptr;                   // partial mat-vec vectors of the tridiagonalisation (one per column chunk)
    double *td_work = nullptr, *td_z = nullptr;   // asb_eig.hip: Householder work vectors / tau / d / e; Z and Q Z
    int64_t td_n = 0;
    // asb_smalldense.hip: tridiagonal eigen-solver, one-sided Jacobi, blocked Cholesky
    double* tri_work = nullptr;
    unsigned char* tri_swp = nullptr;
    double *jac_q = nullptr, *jac_sig = nullptr, *jac_a = nullptr;
    int* jac_where = nullptr;
    double* chol_w = nullptr;
    double* deim_m = nullptr;         // asb_deim_run: Mx, Minv, coef, partials
    long long* deim_pt = nullptr;
    double *eig_lam = nullptr, *eig_v = nullptr;  // asb_sym_eig_topk: eigenvalues (n, descending), leading vectors (n x k)
    int64_t eig_n = 0, eig_k = 0;
    // reconstruction-error sweeps and the held-out animation (asb_recon.hip)
    double* rc_part = nullptr;        // per-block partials of asb_recon_sweep + the reduced row
    int* rc_ks = nullptr;             // sweep points
    int64_t ho_F = 0, ho_Fp = 0;      // held-out frames, padded to 16
    int64_t ho_K = 0;                 // components the held-out factor was built for (0: none yet)
    double* ho_Y = nullptr;           // (3*n_loc, ho_Fp) held-out tensor, transformed like X
    double* ho_Ct = nullptr;          // (3*n_loc, K) transposed basis for the Gram products
    double *ho_P = nullptr, *ho_G = nullptr;      // Y C^T (ho_F x K), C C^T (K x K) when the caller passes no buffers
    double* ho_T = nullptr;           // (K, K) L^-1, rows of dependent components zero
    double* ho_Q = nullptr;           // (K, 3*n_loc) Q = L^-1 C
    double* ho_Zt = nullptr;          // (K, ho_Fp) Z^T = L^-1 P^T
    double* ho_W = nullptr;           // (ho_F, K) least-squares weights on the components
    // interpolation-error sweeps of constraint bases (asb_interp.hip)
    long long* is_idx = nullptr;      // rows to gather
    double* is_B = nullptr;           // (npt, F, 3) rows of the tensor at the interpolation points
    double* is_M = nullptr;           // per sweep point (3, rp, npt): (A^T A)^-1 A^T
    double* is_C = nullptr;           // per sweep point (3, rp, F): the coefficients
    double* is_part = nullptr;        // per-block partials + the reduced row
    long long* is_off = nullptr;      // C offsets per sweep point; M and C offsets per row of C
    int* is_int = nullptr;            // rp per sweep point; npt and coordinate per row of C
    // on-mesh accuracy maps (asb_onmesh.hip)
    int *om_tris = nullptr, *om_ptr = nullptr, *om_star = nullptr;    // triangles (M, 3); vertex-star CSR: offsets (n + 1), triangles
    int64_t om_verts = 0;             // vertices of the uploaded mesh (0: none)
    double* om_invm = nullptr;        // (n_loc) 1 / massL
    double* om_vpart = nullptr;       // (frame tiles, n_loc) per-vertex sums of the error pass
    double* om_fpart = nullptr;       // per block: numerators | denominators of its tile's frames
    double* om_spart = nullptr;       // per block [-min, max, NaN seen]: error pass | normal pass
    double* om_out = nullptr;         // accum_norm | accum_angle | per-frame numerators | denominators | statistics
    double* om_scratch = nullptr;     // (3*n_loc, cw) reconstruction of one chunk of frames
    double *om_fe = nullptr, *om_ang = nullptr;   // (frames, n_loc) maps, only when asked for
    // constraint projections of the resident positions (asb_cproj.hip)
    CpSetup cp;                       // the last asb_cproj_setup (kind -1: none, or a solve's slot took it over)
    double* cp_invm = nullptr;        // (n_loc) 1 / massL
    int *cf_ptr = nullptr, *cf_idx = nullptr;     // asb_cforce_run: the CSR of S^T (n_loc + 1 offsets, columns)
    double* cf_val = nullptr;         // its values
    double* cf_scratch = nullptr;     // (3 * cp.n * p, cw) element-major projections of one chunk of frames
    // reduced constraint forces S^T V (P^T V)^+ P^T p (asb_rforce.hip) and hyper-reduced iterations (asb_pdsolve.hip): the banks of
    // asb_rforce_bank.  rf_bank is the ONLY home of a bank's buffers and numbers, whichever bank is current: a selection sets
    // rf_cur and moves nothing, so a buffer's asb_alloc key (the address of its member here) never changes.  The entry points
    // that address "the current bank" take rf_bank[rf_cur] (asb_rf_cur), a slot of a solve takes rf_bank[slot.bank].
    struct RfBank {
        double* M = nullptr;              // (3, mpp, Np): M_d^T = (S^T V_d)^T, vertices contiguous, zero padding
        int64_t n = 0, Np = 0;            // its vertices; rounded up to the kernel's 32
        int64_t mp = 0, mpp = 0;          // its basis vectors (0: no operator); rounded up to 4
        double* H = nullptr;              // (3, r, npt) the solver H_d = (A^T A + la I)^-1 A^T
        int* pt = nullptr;                // (npt) rows of the sampled elements' stacked projections
        int64_t r = 0, npt = 0, pt_max = -1;      // basis vectors in use (<= mp; 0: no solver), points, largest row
        double* coef = nullptr;           // (3, r rounded up to 4, cw) coefficients of one chunk of frames
        double* G = nullptr;              // G_d^T = (A^-1 M_d)^T in M's layout, (3, mpp, Np) (asb_hyper_operator)
        int ok = 0;                       // G belongs to the current solver and M (a new system matrix clears it in every
                                          // bank, asb_rforce_operator in its own)
        double* Gc = nullptr;             // asb_hyper_iterate: the touched columns of G, (3, mpp, N_t rounded up to 32, zero padding)
        double* Gz = nullptr;             // asb_zroll_operator: (At^-1 U^T M_d)^T, (3, mpp, rq), zero padding
        int zok = 0;                      // Gz belongs to the subspace held and to M: cleared wherever ok is by a set-up or a new M
    };
    RfBank rf_bank[ASB_RFORCE_BANKS];
    int rf_cur = 0;
    double* fd_part = nullptr;        // asb_force_diff: per-frame records + the reduced row
    // global step q = A^-1 rhs (asb_gstep.hip)
    double* gs_Ainv = nullptr;        // (gs_Np, gs_Np) the explicit inverse of A_N, the padding an identity block
    int64_t gs_n = 0, gs_Np = 0;      // its vertices (0: no set-up); rounded up to the kernel's 32
    double* gs_diag = nullptr;        // (n_loc) asb_gstep_inertia: masses / h^2
    asb_pds* pds = nullptr;           // the solve in progress and its buffers (asb_pdsolve.hip)
    // positional constraints (asb_pins_set, asb_pdsolve.hip): checked and uploaded once, read by every later pin term
    struct Pins {
        int64_t P = 0, n = 0, T = 0;      // pins (0: none), the vertices they were checked against, rows of shift (0: fixed pins)
        int per_pin = 0;                  // shift is (T, P, 3) instead of (T, 3)
        int* v = nullptr;                 // (P) vertices, no two equal
        double *wi = nullptr, *p0 = nullptr, *shift = nullptr;        // (P) weights, (P, 3) targets, the shift
    };
    Pins pins;
    // external forces and the floor of the time steps (asb_ext_set, asb_pdsolve.hip): checked and uploaded once, read by
    // asb_pdsolve_external and every advance of a solve they are bound to
    struct Ext {
        int64_t n = 0, T = 0;             // the vertices they were checked against (0: nothing set); rows of fa (0: constant, or no table)
        int force = 0, floor = 0, axis = 1;       // a table is held; the floor is on, along this coordinate
        double height = 0.0;
        double* fa = nullptr;             // (max(T, 1), 3 n) the displacements dt^2 force / mass, row 3 v + d contiguous
    };
    Ext ext;
    // the global step's second solver (asb_gslab.hip): the block-tridiagonal slab factor of A_N.  The context holds EITHER
    // gs_Ainv (gs_n > 0) or the factor (asb_gslab_n(ctx) > 0): each set-up releases the other
    asb_gsl* gsl = nullptr;
    // the third solver (asb_gsub.hip): the step in a position subspace q = o + U z.  One of the three is held at a time
    asb_gsb* gsb = nullptr;
    asb_zr* zr = nullptr;             // the roll-out whose state lives in z (asb_zroll.hip)

    // ---- profiling of the dominant streaming kernel ----
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
};

// projection path entry points (asb_project.hip), dispatched on ctx->mode
int asb_project_begin(asb_ctx* ctx, int64_t K);
long long asb_sketch_capacity(asb_ctx* ctx);       // asb_sketch.hip
int asb_sketch_predict(asb_ctx* ctx, const double* cols, long long stride, const double* wn2, int wn2_stride, const double* E,
                       long long n, int r, int steps);
int asb_project_run(asb_ctx* ctx, int64_t k0, int64_t k1);
void asb_splocs_free(asb_ctx* ctx);
void asb_geo_free(asb_ctx* ctx);
void asb_pdsolve_free(asb_ctx* ctx);
void asb_gslab_free(asb_ctx* ctx);
void asb_gsub_free(asb_ctx* ctx);
void asb_zroll_free(asb_ctx* ctx);
#define ASB_GEO_CACHE_SLABS 64          // x 64 distance fields
const double* asb_geo_cached_field(asb_ctx* ctx, long long slot, long long* n_out);
// small dense linear algebra on the device (asb_linalg.hip)
// out[i*so_i + j*so_j] = sum_r A[r*lda + i*sa] * B[r*ldb + j]   (f64 MFMA; contraction index r slow in A and B)
// I_split > 0: split the contraction as an I_split-row product would (a row shard then sums in the order of the whole)
int asb_gemm_tn_s(asb_ctx* ctx, const double* A, long long lda, long long sa, const double* B, long long ldb, long long Rn,
                  int I, int J, double* out, long long so_i, long long so_j, long long I_split = 0);
static inline int asb_gemm_tn(asb_ctx* ctx, const double* A, long long lda, const double* B, long long ldb, long long Rn,
                              int I, int J, double* out) {
    return asb_gemm_tn_s(ctx, A, lda, 1, B, ldb, Rn, I, J, out, J, 1);
}
int asb_transpose(asb_ctx* ctx, const double* in, long long rows, long long cols, double* out);   // (rows x cols) -> (cols x rows)
// eigen-decomposition of a symmetric n x n matrix (n <= 128) on the device: lam (n) descending, V (n x n) columns
int asb_sym_eig(asb_ctx* ctx, const double* A_dev, int n, double* lam_dev, double* V_dev);
// asb_smalldense.hip
int asb_tri_eig_dev(asb_ctx* ctx, const double* d, const double* e, int n, int k, double* lam_desc, double* Z, int* n_bad);
int asb_jacobi_rows_dev(asb_ctx* ctx, double* A, int nv, int m, long long lda, double* Q_sorted, int q_transposed,
                        double* sig_sorted, int* sweeps_out);
int asb_sym_eig_large(asb_ctx* ctx, const double* A_dev, int n, double* lam_dev, double* V_dev);
int asb_chol_tinv_dev(asb_ctx* ctx, const double* G, int K, double* Tt, int* status_dev);
int asb_components_transform_dev(asb_ctx* ctx, const double* T_dev, int same_T);      // asb_linalg.hip
int asb_project_results(asb_ctx* ctx, double* comps, double* weigs, int64_t* idx, double* sigma, double* normR2_local);

#define ASB_FAIL(ctx, code, ...)                                   \
    do {                                                           \
        char _b[512];                                              \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                     \
        (ctx)->err = _b;                                           \
        return (code);                                             \
    } while (0)

#define ASB_HIP(ctx, call)                                                                   \
    do {                                                                                     \
        hipError_t _e = (call);                                                              \
        if (_e != hipSuccess)                                                                \
            ASB_FAIL(ctx, ASB_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), \
                     __FILE__, __LINE__);                                                    \
    } while (0)

// C = beta C + alpha A B (row-major, even dimensions; asb_dense.hip) and the in-place SPD inverse built on it
bool asb_combine_rows_ok(const asb_ctx* ctx);          // asb_linalg.hip
int asb_combine_rows(asb_ctx* ctx, const double* T_dev);
int asb_gemm_nn(asb_ctx* ctx, const double* A, long long lda, const double* B, long long ldb, double* C, long long ldc, int M,
                int N, int Kc, double alpha, double beta, int tri = 0);
int asb_dense_spd_inverse(asb_ctx* ctx, double* M, int np);
int asb_deflate_apply_dev(asb_ctx* ctx, int64_t k, const double* s_dev);      // asb_deflate.hip
// G = X^T X (n x n, both triangles) for a tall row-major X: LDS-tiled f64 MFMA kernel (asb_linalg.hip)
int asb_syrk_tn(asb_ctx* ctx, const double* X, long long ld, long long R, int n, double* out);
int asb_gemm_tn_big(asb_ctx* ctx, const double* X, long long ldx, const double* Y, long long ldy, long long R, int I, int J, double* out);
#define ASB_CHECK_LAUNCH(ctx) ASB_HIP(ctx, hipGetLastError())
// asb_cproj.hip, shared with asb_rforce.hip.  The checks of the arguments asb_cproj_run shares with its siblings (messages start
// with `who`) and the world of the selected tensor, without the mass factors; n_sel: the frames range(f0, f1, fj) selects
int asb_cproj_world(asb_ctx* ctx, const char* who, int which, int64_t f0, int64_t f1, int64_t fj, int add_mean, double psf,
                    double sigma_min, double sigma_max, CpWorld* w, int64_t* n_sel);
// its part that needs no element set-up: the tensor of `which`, the frame range, the mean and the scale checked, w filled
int asb_world_frames(asb_ctx* ctx, const char* who, int which, int64_t f0, int64_t f1, int64_t fj, int add_mean, double psf, CpWorld* w,
                     int64_t* n_sel);
// the first device work of a call, after all of its checks: inv_massL (host, or NULL) uploaded and put into w
int asb_cproj_invm(asb_ctx* ctx, const double* inv_massL, CpWorld* w);
// selected frames [c0, c0 + cn) projected ELEMENT-major into S (3 cp.n p rows of cw doubles) for the element set-up cp: the
// context's (ctx->cp) or a slot's
void asb_cproj_em_launch(asb_ctx* ctx, const CpSetup& cp, const CpWorld& w, int f0, int fj, int c0, int cn, int cw, double smin, double smax,
                         double* S);
// rows of the stacked projections of a set-up of `kind` with n_elem elements
long long asb_cproj_rows(int kind, long long n_elem);
// the chunk width of asb_cforce_run for projections of n_cols rows, and one chunk's k_st_apply on a device CSR
long long asb_cforce_chunk_width(long long n_cols, long long chunk_frames, long long n_sel);
void asb_st_apply_launch(asb_ctx* ctx, const int* ptr, const int* ci, const double* val, const double* S, int cw, int c0, int cn,
                         long long n_rows, int accumulate, double* out);
// asb_rforce.hip, the banks of asb_rforce_bank (asb_ctx::rf_bank).  asb_rf_cur: the bank the entry points address now;
// asb_rf_invalidate_all clears the A^-1 S^T V mark of every bank (a new system matrix)
static inline asb_ctx::RfBank& asb_rf_cur(asb_ctx* ctx) { return ctx->rf_bank[ctx->rf_cur]; }
void asb_rf_invalidate_all(asb_ctx* ctx);
// the chunk width of asb_rforce_run for a solver of r basis vectors and sampled projections of n_cols rows; one chunk's
// k_rforce_coef and k_rforce_gemm with the operator and solver of `bank`, from the element-major projections S (coefficients
// into bank.coef, which the caller has sized)
long long asb_rforce_chunk_width(long long r, long long n_cols, long long n_sel);
void asb_rforce_chunk_launch(asb_ctx* ctx, const asb_ctx::RfBank& bank, const double* S, int cw, int c0, int cn, int accumulate, double* out);
// its first half alone: k_rforce_coef of one chunk into bank.coef ((3, r rounded up to 4, cw), zero past row r and frame cn)
void asb_rforce_coef_launch(asb_ctx* ctx, const asb_ctx::RfBank& bank, const double* S, int cw, int cn);
// asb_gstep.hip: k_gs_inertia on device arrays; add: out += diag s, otherwise out = diag s (the value the sum adds)
void asb_gs_inertia_launch(asb_ctx* ctx, const CpWorld& w, int f0, int fj, int n_sel, long long n, const double* diag_dev, int mode,
                           const double* acc3, bool add, double* out);
// asb_gstep.hip: the checks of a system matrix that asb_gstep_setup and asb_gslab_setup share, messages starting with `who`:
// the tensor on the device has n vertices (one rank), asb_csr_check32, finite values, a positive diagonal, a symmetric pattern
// and values symmetric to 1e-12 of the row's largest
int asb_gs_check_matrix(asb_ctx* ctx, const char* who, int64_t n, const int64_t* indptr, const int64_t* indices, const double* data,
                        std::vector<int>& p32, std::vector<int>& c32);
// asb_gslab.hip.  asb_gslab_n: the vertices of the slab factor the context holds (0: none); asb_gslab_release: the factor
// and its work matrices are freed (asb_gstep_setup calls it: the context holds one solver)
long long asb_gslab_n(const asb_ctx* ctx);
void asb_gslab_release(asb_ctx* ctx);
// A^-1 applied through the factor, all in stream order, nothing synchronised.  solve_fm: rhs (F, n, 3) frame-major -> Qv (3 n, ld)
// vertex-major, ld = F rounded up to 64 (columns [F, ld) of Qv are written as zero); Qv NULL: a buffer of the factor.  out
// (optional): the same values frame-major (F, n, 3)
int asb_gslab_solve_fm(asb_ctx* ctx, const double* rhs, long long F, double* Qv, double* out);
// Gt (rows, Np) with the n vertices contiguous in a row (the layout of RfBank::M) -> Ot, same layout: Ot[r] = A^-1 Gt[r]; the
// entries of Ot past vertex n are left as they are
int asb_gslab_solve_rows(asb_ctx* ctx, const double* Gt, long long rows, long long Np, double* Ot);
// asb_gsub.hip, the roles of the asb_gslab_* calls above for the position subspace q = o + U z.  asb_gsub_n: the vertices of the
// subspace the context holds (0: none); asb_gsub_release: freed (every other set-up calls it).  solve_fm: the AFFINE map
// o' + P rhs with the arguments of asb_gslab_solve_fm (columns [F, ld) of Qv are not written); solve_rows: the LINEAR part P Gt[r]
// alone, with the arguments of asb_gslab_solve_rows (Np: the subspace's padding, rows = 3 mpp <= 65535)
long long asb_gsub_n(const asb_ctx* ctx);
void asb_gsub_release(asb_ctx* ctx);
int asb_gsub_solve_fm(asb_ctx* ctx, const double* rhs, long long F, double* Qv, double* out);
int asb_gsub_solve_rows(asb_ctx* ctx, const double* Gt, long long rows, long long Np, double* Ot);
// what asb_zroll.hip takes from the subspace: its numbers and buffers (Un: U in W's layout (3, Np, rq); o, Ao (n, 3)); 0: none held
struct GsubView {
    long long n, r, rp, rq, Np, gen;    // gen: one number per asb_gsub_setup
    const double *Ut, *Wn, *Un, *o, *Ao;
};
int asb_gsub_view(asb_ctx* ctx, GsubView* v);
// the work matrices R (3 Np, ld; rows past 3 n zero) and Y (3, rq, ld) for rows of ld doubles; Y = W R (basis 1: U^T R) into Y
int asb_gsub_work(asb_ctx* ctx, long long ld, double** R, double** Y);
void asb_gsub_reduce_launch(asb_ctx* ctx, int basis, long long ld, double* Y);
// k_gsub_expand on a basis Ut (3, rp, Np) of the subspace's r (gathered rows: any Np a multiple of 32): Q (3 n, ld) = base (n, 3)
// + U Y, columns [0, F); out (optional): the same frame-major
void asb_gsub_expand_launch(asb_ctx* ctx, const double* Ut, long long Np, const double* Y, long long ld, const double* base, double* Q,
                            long long F, long long n, double* out);
// the first half of asb_gsub_solve_rows: Y (3, rq, ld) = W Mt^T for the operator rows Mt (3 mpp, Np), ld = mpp rounded up to 64
int asb_gsub_rows_in(asb_ctx* ctx, const double* Mt, long long rows, long long Np, long long* ld_out, double** Y);
// asb_rforce.hip: k_st_dense on device arrays, Mt (3, mpp, Np) = (S^T V_d)^T for the CSR (ptr, ci, val) of n_rows rows and V (rows, mp, 3)
void asb_st_dense_launch(asb_ctx* ctx, const int* ptr, const int* ci, const double* val, const double* V, long long n_rows, int mp, int mpp,
                         long long Np, double* Mt);
// asb_rforce.hip, the record of asb_force_diff for one frame / for all: [0..2] sum (a - b)^2 per axis, [3..5] sum a^2 per axis,
// [6] max |a - b|, [7] max a.  asb_force_diff_final_launch: rec[F] = the records rec[0 .. F) combined (k_force_diff_final)
#define FD_REC 8
__device__ __forceinline__ void fd_combine(double (&x)[FD_REC], const double* y) {
#pragma unroll
    for (int q = 0; q < 6; ++q) x[q] += y[q];
    x[6] = fmax(x[6], y[6]);
    x[7] = fmax(x[7], y[7]);
}
void asb_force_diff_final_launch(asb_ctx* ctx, double* rec, long long F);
// the host's side of asb_force_diff: rec ((F + 1) x FD_REC, device) read back behind the stream and handed out
int asb_force_diff_outputs(asb_ctx* ctx, const double* rec_dev, long long F, double* sums_out, double* max_out, double* norms_out,
                           double* per_frame_out);
// asb_pdsolve.hip: k_pd_untranspose, P (rows, ld) vertex-major -> out (n_sel, rows) frame-major; k_pd_transpose, the other way
void asb_pd_untranspose_launch(asb_ctx* ctx, const double* P, int n_sel, long long rows, long long ld, double* out);
void asb_pd_transpose_launch(asb_ctx* ctx, const double* in, int n_sel, long long rows, double* Q, long long ld);
// a host CSR checked (offsets from 0 and not decreasing, columns < n_cols and strictly ascending in a row) and narrowed to int;
// `what` names the matrix in the messages
int asb_csr_check32(asb_ctx* ctx, const char* who, int64_t n_rows, const int64_t* indptr, const int64_t* indices, const double* data,
                    long long n_cols, std::vector<int>& p32, std::vector<int>& c32, const char* what = "S^T");
// the CSR it narrowed, copied on the context's stream into device arrays the caller owns: dptr of p32.size() ints, dci and
// dval of c32.size() + 1 entries (no empty allocation for a matrix without entries).  Nothing is allocated or synchronised here: the caller drains the stream
// before the vectors die
static inline int asb_csr_stage(asb_ctx* ctx, const std::vector<int>& p32, const std::vector<int>& c32, const double* data, int* dptr,
                                int* dci, double* dval) {
    ASB_HIP(ctx, hipMemcpyAsync(dptr, p32.data(), p32.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    if (!c32.empty()) {
        ASB_HIP(ctx, hipMemcpyAsync(dci, c32.data(), c32.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        ASB_HIP(ctx, hipMemcpyAsync(dval, data, c32.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    return ASB_OK;
}

// ASB_DEBUG_PANELS: the panel loop's trace on stderr (changes no result); read once per process
static inline bool asb_debug_panels() {
    static const bool on = getenv("ASB_DEBUG_PANELS") != nullptr;
    return on;
}

// 1 KiB of pinned host memory shared by the small per-panel / per-sweep read-backs:
//   [0, 256) PanelState, [256, 272) panel-kernel flags, [384, 392) counters, [448, 456) publication sequence number
static inline int asb_pin_alloc(asb_ctx* ctx) {
    if (ctx->host_pin) return ASB_OK;
    ASB_HIP(ctx, hipHostMalloc((void**)&ctx->host_pin, 1024, hipHostMallocCoherent | hipHostMallocMapped));
    for (int i = 0; i < 1024; ++i) ctx->host_pin[i] = 0;
    if (hipHostGetDevicePointer((void**)&ctx->host_pin_dev, ctx->host_pin, 0) != hipSuccess) ctx->host_pin_dev = nullptr;
    return ASB_OK;
}

// Context-owned device buffers are registered in ctx->alloc_bytes under the address of their owning pointer (`slot`), here
// alone.  asb_capacity: the elements registered for *slot (0: none); asb_release: freed, key erased; _all: asb_destroy
template <typename T>
static inline size_t asb_capacity(const asb_ctx* ctx, T* const* slot) {
    auto it = ctx->alloc_bytes.find((void*)slot);
    return *slot && it != ctx->alloc_bytes.end() ? it->second / sizeof(T) : 0;
}
template <typename T>
static inline void asb_release(asb_ctx* ctx, T** slot) {
    (void)hipFree(*slot);
    *slot = nullptr;
    ctx->alloc_bytes.erase((void*)slot);
}
static inline void asb_release_all(asb_ctx* ctx) {
    while (!ctx->alloc_bytes.empty()) asb_release(ctx, (void**)ctx->alloc_bytes.begin()->first);
}

// (Re)allocates *p to hold `count` elements; an existing allocation that is already large
// enough (and not more than 2x too large) is kept, so repeated runs on one context do not
// pay hipMalloc/hipFree inside a timed region.
template <typename T>
static inline int asb_alloc(asb_ctx* ctx, T** p, size_t count) {
    const size_t want = count * sizeof(T);
    auto it = ctx->alloc_bytes.find((void*)p);
    if (*p && it != ctx->alloc_bytes.end() && it->second >= want && it->second <= 2 * want + 4096) return ASB_OK;
    if (*p) asb_release(ctx, p);
    if (count == 0) return ASB_OK;
    ASB_HIP(ctx, hipMalloc((void**)p, want));
    ctx->alloc_bytes[(void*)p] = want;
    return ASB_OK;
}

// two context-owned buffers change places, with their registered capacities (both owners live inside the context or its
// solve).  A capacity is keyed on the address of the owning pointer, so this is the one place where a key follows a buffer;
// its only user is asb_cp_move below
template <typename T>
static inline void asb_swap_buf(asb_ctx* ctx, T** a, T** b) {
    auto cap = [&](void* key) {
        auto it = ctx->alloc_bytes.find(key);
        const size_t c = it == ctx->alloc_bytes.end() ? 0 : it->second;
        if (it != ctx->alloc_bytes.end()) ctx->alloc_bytes.erase(it);
        return c;
    };
    const size_t ca = cap((void*)a), cb = cap((void*)b);
    std::swap(*a, *b);
    if (*a) ctx->alloc_bytes[(void*)a] = cb;
    if (*b) ctx->alloc_bytes[(void*)b] = ca;
}

// An element set-up changes owner, the context to a slot of a solve: pointers, no copy.  `to`'s previous buffers pass to
// `from` (its next asb_cproj_setup reuses them), which has no set-up afterwards
static inline void asb_cp_move(asb_ctx* ctx, CpSetup& from, CpSetup& to) {
    asb_swap_buf(ctx, &from.idx, &to.idx);
    asb_swap_buf(ctx, &from.table, &to.table);
    asb_swap_buf(ctx, &from.sptr, &to.sptr);
    asb_swap_buf(ctx, &from.sidx, &to.sidx);
    to.kind = from.kind, to.n = from.n, to.verts = from.verts, to.vmax = from.vmax;
    from.kind = -1;
}

// A device buffer that lives inside one call: freed when it goes out of scope (hipFree waits for the device, so work still in
// flight on the buffer is safe), unless asb_adopt has handed it to the context.  Buffers that outlive a call go through asb_alloc.
template <typename T>
struct asb_tmp {
    asb_tmp() = default;
    asb_tmp(const asb_tmp&) = delete;
    asb_tmp& operator=(const asb_tmp&) = delete;
    ~asb_tmp() { if (p) (void)hipFree(p); }
    int alloc(asb_ctx* ctx, size_t count) {          // (an earlier allocation of this owner is freed first)
        if (p) (void)hipFree(p);
        p = nullptr;
        ASB_HIP(ctx, hipMalloc((void**)&p, count * sizeof(T)));
        return ASB_OK;
    }
    T* get() const { return p; }
    T* release() { T* q = p; p = nullptr; return q; }

private:
    T* p = nullptr;
};

// The filled temporary becomes *slot's registered buffer of `count` elements; the previous one is freed
template <typename T>
static inline void asb_adopt(asb_ctx* ctx, T** slot, asb_tmp<T>& buf, size_t count) {
    asb_release(ctx, slot);
    *slot = buf.release();
    ctx->alloc_bytes[(void*)slot] = count * sizeof(T);
}
// *p gets room for count_new elements and keeps its first count_keep: a buffer that is large enough stays (no upper bound),
// otherwise a new one is filled by a copy, drained and adopted.  A failure leaves the old buffer in place (message: `who`)
template <typename T>
static inline int asb_grow_keep(asb_ctx* ctx, const char* who, T** p, size_t count_new, size_t count_keep) {
    if (*p && asb_capacity(ctx, p) >= count_new) return ASB_OK;
    asb_tmp<T> q;
    int rc;
    if ((rc = q.alloc(ctx, count_new))) return rc;
    if (*p && count_keep) {
        hipError_t e = hipMemcpyAsync(q.get(), *p, count_keep * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) ASB_FAIL(ctx, ASB_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    }
    asb_adopt(ctx, p, q, count_new);
    return ASB_OK;
}

// The POD in levels (asb_pod.hip): a level is open while X views X_lvl; asb_pod_deflate_end and every ingest call drop it
static inline bool asb_pod_level_open(const asb_ctx* ctx) { return ctx->X != ctx->X_in; }
static inline void asb_pod_level_drop(asb_ctx* ctx) {
    ctx->X = ctx->X_in;
    asb_release(ctx, &ctx->X_lvl);
    asb_release(ctx, &ctx->pod_u1);
    ctx->pod_u1_rows = 0;
}

// asb_recon.hip: what asb_recon_sweep and asb_onmesh_run read for `which` -- 0: the training tensor, the greedy weights, the
// device basis; 1: the held-out tensor, Z^T, Q -- checked for `kmax` components (messages: "who: idx = ...")
struct RcOperands { const double *T, *A, *B; long long ldt, lda; int F; };
int asb_recon_operands(asb_ctx* ctx, const char* who, const char* idx, int which, int64_t kmax, RcOperands* o);

// asb_snapshots.hip: the shard [v0, v0 + n_loc) of a host tensor (F, N_glob, 3) and of its mass vector, staged on the device
int asb_stage_shard(asb_ctx* ctx, const double* X, int64_t F, int64_t N_glob, int64_t v0, int64_t n_loc, const double* massL,
                    asb_tmp<double>& stage, asb_tmp<double>& mdev);
// test hooks on host arrays (asb_linalg.hip): a device copy of n host doubles (nullptr: NaN) with `slack` NaN behind it; the
// copy back of out_len doubles after the stream drains (rc: the status so far, passed through)
int asb_test_stage(asb_ctx* ctx, const double* h, size_t n, size_t slack, asb_tmp<double>& d);
int asb_test_finish(asb_ctx* ctx, int rc, const double* out_dev, double* out_host, size_t out_len);

int asb_dl_begin(asb_ctx* ctx);          // asb_linalg.hip
// component rows [dl_done, k_to) are final: copy them to the pinned buffer on the copy stream, behind what the main stream
// has enqueued so far (no-op unless asb_components_stream is on)
static inline int asb_dl_enqueue(asb_ctx* ctx, long long k_to) {
    if (!ctx->dl_enabled || !ctx->dl_host || !ctx->comps || k_to <= ctx->dl_done) return ASB_OK;
    if (k_to > ctx->K) k_to = ctx->K;
    const size_t row = (size_t)3 * ctx->n_loc;
    if ((size_t)k_to * row > ctx->dl_host_count) return ASB_OK;
    ASB_HIP(ctx, hipEventRecord(ctx->dl_event, ctx->stream));
    ASB_HIP(ctx, hipStreamWaitEvent(ctx->dl_stream, ctx->dl_event, 0));
    ASB_HIP(ctx, hipMemcpyAsync(ctx->dl_host + (size_t)ctx->dl_done * row, ctx->comps + (size_t)ctx->dl_done * row,
                                (size_t)(k_to - ctx->dl_done) * row * sizeof(double), hipMemcpyDeviceToHost, ctx->dl_stream));
    ctx->dl_done = k_to;
    return ASB_OK;
}

// ---------------------------------------------------------------- device helpers
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// Wave-wide reductions without the LDS crossbar (gfx950): four DPP stages inside a row of 16 lanes (quad_perm xor 1, xor 2,
// row_half_mirror, row_mirror), then v_permlane16_swap / v_permlane32_swap across rows -- a stage is two 32-bit moves and an
// add instead of two ds_bpermute round trips (~6 x 120 cycles for a butterfly of __shfl_xor).  Every stage combines two
// values that are each identical in the lanes they come from, so all 64 lanes end with bit-identical results.
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
// the two values a lane sees after the swap: (own, partner) for rows (16) / halves (32)
__device__ __forceinline__ void swap16_f64(double v, double& a, double& b) {
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    a = __hiloint2double((int)h[0], (int)l[0]);
    b = __hiloint2double((int)h[1], (int)l[1]);
}
__device__ __forceinline__ void swap32_f64(double v, double& a, double& b) {
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    a = __hiloint2double((int)h[0], (int)l[0]);
    b = __hiloint2double((int)h[1], (int)l[1]);
}
template <int NV>
__device__ __forceinline__ void wave_sum_dpp(double (&v)[NV]) {
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] += dpp_mov_f64<0xB1>(v[q]);
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] += dpp_mov_f64<0x4E>(v[q]);
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] += dpp_mov_f64<0x141>(v[q]);
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] += dpp_mov_f64<0x140>(v[q]);
#pragma unroll
    for (int q = 0; q < NV; ++q) { double a, b; swap16_f64(v[q], a, b); v[q] = a + b; }
#pragma unroll
    for (int q = 0; q < NV; ++q) { double a, b; swap32_f64(v[q], a, b); v[q] = a + b; }
}
__device__ __forceinline__ double wave_max_dpp(double v) {
    v = fmax(v, dpp_mov_f64<0xB1>(v));
    v = fmax(v, dpp_mov_f64<0x4E>(v));
    v = fmax(v, dpp_mov_f64<0x141>(v));
    v = fmax(v, dpp_mov_f64<0x140>(v));
    double a, b;
    swap16_f64(v, a, b); v = fmax(a, b);
    swap32_f64(v, a, b); v = fmax(a, b);
    return v;
}
__device__ __forceinline__ int wave_min_dpp(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true));
    v = min(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true));
    auto s = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    v = min((int)s[0], (int)s[1]);
    s = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    return min((int)s[0], (int)s[1]);
}

__device__ __forceinline__ int wave_isum_dpp(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);
    auto s = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    v = (int)s[0] + (int)s[1];
    s = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    return (int)s[0] + (int)s[1];
}

// Block-wide sum of NV values per thread; result valid in every thread.
// scratch: at least NV * (blockDim.x/64) doubles of LDS.
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* scratch) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    if (nw == 1) return;
    __syncthreads();
    if (lane == 0)
        for (int i = 0; i < NV; ++i) scratch[wid * NV + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        double s = 0;
        for (int w = 0; w < nw; ++w) s += scratch[w * NV + i];
        v[i] = s;
    }
}

// "better" for arg-max with NumPy's first-max tie-break: larger value, then lower index.
__device__ __forceinline__ bool am_better(double e, long long i, double be, long long bi) {
    return (e > be) || (e == be && i < bi);
}
