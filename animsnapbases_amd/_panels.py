"""Projection-mode ("panel") deflation over several ranks -- shared by posComponents (vertex rows) and
constraintsComponents 'pca_blocks' with p = 1 (constraint rows)."""
import os

import numpy as np


def _on(name):
    return os.environ.get(name, "1") != "0"


def _residual_rest(eng, comm, k0, K):
    """Components k0 .. K - 1 through the residual protocol (posComponents.py:76-96 as is: one all-gather of
    [energy, idx, 3 x F slab] records per component) -- where a run ends up that left the projection mode."""
    rec = recs = None
    if comm.multi:
        rec, recs = comm.new_records(eng.xchg_len(), eng.device_exchange)
    for k in range(k0, K):
        if comm.multi:
            eng.local_best(k, rec.data_ptr())
            comm.all_gather_records(rec, recs)
            eng.pick(k, recs.data_ptr(), comm.world)
        else:
            eng.pick(k)
        eng.apply(k)


class _Run(object):
    """One run of the driver: what is fixed at its start (exchange buffers, which protocols are on) and what changes from
    read to read (k, the stall counters, the budgets).  Every decision field holds the same value on all ranks."""

    def __init__(self, eng, comm, n_rows, K):
        self.eng, self.comm, self.K = eng, comm, K
        dev = self.dev = comm.exchange_device(eng.device_exchange)
        torch = self.torch = comm._torch
        cap, rl = self.cap, self.rl = eng.panel_capacity(), eng.panel_row_len()
        _, e0 = eng.panel_scale()
        # ONE start-up exchange: the largest initial energy (histogram range and rounding margin must be the same everywhere) and
        # what decides the guessed first panel travel together, as bit patterns in one all-gather of four words per rank
        # (an engine that exchanges through host memory is the CPU test double: it has neither the guessed first panel nor the
        # switch to the residual loop, and with it neither the device word, the co-resident kernel nor sub-panels below are on)
        gs = (0.0, 0.0, True)
        want_guess = eng.device_exchange and _on("ASB_FIRST_PANEL_MEAN")
        if want_guess:
            gs = eng.panel_guess_stats()
        start = np.array([e0, gs[0], gs[1], 0.0 if gs[2] else 1.0], dtype=np.float64)
        allst = comm.all_gather_ints(start.view(np.int64)).view(np.float64).reshape(-1, 4)
        eng.panel_scale(set_e0max=float(allst[:, 0].max()))
        # exchange buffers, kept on the engine between calls (49 MB: allocating and clearing them cost 1.3 ms per call).
        # Nothing reads the padding: the assembly takes counts[r] rows of rank r's piece.
        key = (cap, rl, comm.world, str(dev))
        bufs = getattr(eng, "_panel_bufs", None)
        if bufs is None or bufs[0] != key:
            eng._panel_bufs = (key, torch.empty(cap * (rl + 1), dtype=torch.float64, device=dev),   # rows, then (packed exchange) the ids
                               torch.empty(cap, dtype=torch.int64, device=dev),
                               torch.empty(cap + 1, dtype=torch.float64, device=dev),
                               torch.empty(comm.world * (cap + 1), dtype=torch.float64, device=dev))
        _, self.rows_loc, self.idx_loc, self.top_loc, self.top_all = eng._panel_bufs
        # counts of a pass stay on the device (min over the ranks, ONE read) when the exchange tensors do
        self.spec_word = torch.zeros(1, dtype=torch.float64, device=dev) if dev.type != "cpu" else None
        on_device = self.spec_word is not None
        # the reduced word comes back through the engine's polled pinned slot when the collective ran on the engine's stream
        # (a communicator that cannot say so -- or an engine on another stream -- gets the synchronising read)
        oes = getattr(comm, "on_engine_stream", None)
        self.same_stream = on_device and bool(oes(eng) if callable(oes) else oes)
        # the co-resident panel kernel (the library says whether it can run at all: not above its frame limit, where every
        # panel takes the two-kernel loop): its lock-step protection over several ranks (see _read_plain) ...
        coop = on_device and eng.panel_coop_possible() and _on("ASB_PANEL_COOP")
        self.coop_check = bool(coop and comm.multi)
        # ... and several sub-panels per read of X in one launch and one exchange (see _read_one_launch)
        self.multi_sub = bool(coop and _on("ASB_DOUBLE_PANELS"))
        self.words = torch.zeros(10, dtype=torch.float64, device=dev) if self.multi_sub else None
        self.sub_max = max(1, min(4, int(os.environ.get("ASB_SUB_PANELS", "4"))))
        self.sub_cur = min(self.sub_max, max(1, int(os.environ.get("ASB_SUB_FIRST", "4"))))
        self.sub_budget = [16] * 8
        self.global_all = n_rows <= cap
        self.spec_budget = 16 if _on("ASB_SPEC_PANELS") else 0
        # first panel guessed from the energies without the constant-in-time direction (asb.h: asb_panel_guess_*): a collective
        # decision -- every rank must be able to, and the share of that direction in |X|^2 over ALL shards must exceed 1/4
        self.guess_ok = False
        if self.spec_budget and not self.global_all and want_guess:
            tot = allst[:, 1:].sum(axis=0)
            self.guess_ok = bool(tot[2] == 0 and tot[1] > 0 and tot[0] > 0.25 * tot[1])
        self.guessing = False
        # the stall rule of the single-rank driver (asb.h: asb_project_switch_residual): reads of X that commit fewer than 3/4 of a
        # component each (K beyond the numerical rank: every panel ends in a refresh) -- the run continues in the residual protocol
        self.stall_rule = eng.device_exchange and _on("ASB_STALL_FALLBACK")
        self.mark_reads = self.mark_k = self.reads = 0
        self.k, self.stalled, self.forced_next = 0, 0, -1

    def read_word(self):
        return self.eng.fetch_double(self.spec_word.data_ptr()) if self.same_stream else self.spec_word.item()

    def leave_kernel(self):
        """Somewhere the kernel's exchange timed out: ALL ranks switch it off (unproven steps, and with them the guess, need
        it); the caller repeats the panel."""
        self.eng.panel_set_coop(False)
        self.coop_check = self.multi_sub = self.guess_ok = False

    def adapt_spec(self, gain):
        # a kept step saves 1/16 of a panel, a rejected one costs one step of the panel kernel: back off only after
        # complete failures
        self.spec_budget = 16 if gain > 0 else max(2, self.spec_budget // 2)


def _candidates(run, forced, take_all):
    """Selects this rank's candidates and replicates the candidate rows of all ranks on every rank: local thresholds, ONE
    all-gather of energies, the global threshold, the selection, ONE all-gather of rows and ids.  True iff candidates were
    assembled (there are some, and no more than the capacity)."""
    eng, comm, torch, k = run.eng, run.comm, run.torch, run.k
    cap, rl, rows_loc, idx_loc = run.cap, run.rl, run.rows_loc, run.idx_loc
    packed = overflow = False
    if not take_all:
        if run.guess_ok and k == 0 and run.stalled == 0:
            eng.panel_guess_begin(comm.world)
            run.guessing = True
        for level in (1, 2):                         # local threshold: ~m_target of this rank's vertices above it
            eng.panel_hist(level, None)
            eng.panel_tau(level, None)
        eng.panel_top_energies(run.top_loc.data_ptr(), cap)
        comm.all_gather_into(run.top_all, run.top_loc)
        counts = eng.panel_global_tau(run.top_all.data_ptr(), comm.world, cap)      # tau installed; the panel's first host sync
        if counts is None:                            # table too large for the selection kernel: same rule with torch
            tab = run.top_all.view(comm.world, cap + 1)
            exported = tab[:, :cap].reshape(-1)
            kth = torch.topk(exported, eng.panel_target() + 1).values[-1].clamp(min=0.0)
            tau = torch.maximum(kth, tab[:, cap].max()).reshape(1).contiguous()
            eng.panel_set_tau(tau.data_ptr())
            counts = (tab[:, :cap] > tau).sum(dim=1).cpu().numpy().astype(np.int64)
        packed = not run.guessing and 0 < int(counts.sum()) <= cap
    if take_all or run.guessing:    # the counts are not in the gathered energies (a guess: the union's size): one more small exchange
        n_c, ov = eng.panel_select(k, rows_loc.data_ptr(), idx_loc.data_ptr(), forced, take_all)
        info = comm.all_gather_ints([n_c, int(ov)])
        counts, overflow = info[:, 0].copy(), bool(info[:, 1].any())
    else:                           # packed: the ids go right behind this rank's maxc rows, both travel in ONE all-gather
        ids_ptr = rows_loc.data_ptr() + 8 * int(counts.max()) * rl if packed else idx_loc.data_ptr()
        eng.panel_select(k, rows_loc.data_ptr(), ids_ptr, -1, False, want_counts=False)
    if overflow or not 0 < int(counts.sum()) <= cap:
        return False
    maxc = int(counts.max())
    if packed:
        piece = maxc * (rl + 1)
        buf_g = torch.empty(comm.world * piece, dtype=torch.float64, device=run.dev)
        comm.all_gather_into(buf_g, rows_loc[:piece])
        eng.panel_assemble_packed(buf_g.data_ptr(), counts, maxc)
    else:
        rows_g = torch.empty(comm.world * maxc * rl, dtype=torch.float64, device=run.dev)
        idx_g = torch.empty(comm.world * maxc, dtype=torch.int64, device=run.dev)
        comm.all_gather_into(rows_g, rows_loc[:maxc * rl])
        comm.all_gather_into(idx_g, idx_loc[:maxc])
        eng.panel_assemble(rows_g.data_ptr(), idx_g.data_ptr(), counts, maxc)
    return True


def _read_one_launch(run):
    """Several sub-panels per read of X (what the single-rank driver does inside the library): ONE launch of the panel kernel
    for all sub-panels of the read (every rank holds the same candidates, so the runs and their nine-word summary are
    identical everywhere), this shard's pass and the checks of all its tiles enqueued behind it, ONE min-all-reduce of the
    per-tile counts (+ the kernel's status) for the whole read, one host read (asb.h: asb_panel_read_run / _commit).  Per read
    of X: two all-gathers (energies; rows + ids) and this all-reduce.
    Returns the components committed; None: the kernel timed out on some rank, the panel again the plain way."""
    eng, words = run.eng, run.words
    nt, ncs, provs = eng.panel_read_run(run.k, run.K, run.sub_cur, run.spec_budget, run.sub_budget, words.data_ptr())
    run.comm.allreduce_min_tensor(words[:9])
    w10 = eng.fetch_doubles(words.data_ptr(), 10) if run.same_stream else words.cpu().numpy()
    if w10[8] < 0:
        w10[:9] = 0.0
        eng.panel_read_commit(w10)                # (rolls back what this shard's local chain adopted; commits nothing)
        run.leave_kernel()
        return None
    total, full, rejected = eng.panel_read_commit(w10)
    if nt > 0:
        # the next read: later sub-panels get as many steps as the last ones kept (+2); twice as many sub-panels after a
        # read whose sub-panels all stood, what stood (+1) after a rejection
        for ct in range(1, min(nt, full + 1)):
            run.sub_budget[ct] = min(16, max(4, int(w10[ct]) + 2))
        if rejected:
            run.sub_cur = min(run.sub_max, full + 1)
        elif nt == run.sub_cur:
            run.sub_cur = min(run.sub_max, 2 * run.sub_cur)
        run.adapt_spec(total - provs[0])
    return total


def _read_plain(run, steps, take_all):
    """One panel per read of X: the panel kernel (or the two-kernel loop), then the pass.  A tail of unproven steps is checked
    by the pass on every shard and the min over the ranks stands (panel_project_spec[_dev] -> all-reduce -> panel_commit);
    provable steps need no exchange.  Returns the components committed.
    The co-resident panel kernel can time out on ONE rank (its GPU shared with other work).  Every rank must then redo the
    panel the same way -- the two-kernel loop, whose steps are the provable ones -- or the ranks fall out of lock-step.  While
    that check is on, the status rides on the min all-reduce that panels with unproven steps need anyway: a rank whose launch
    failed contributes -1 (and skips its pass)."""
    eng, comm, k, spec_word = run.eng, run.comm, run.k, run.spec_word
    while True:
        if run.spec_budget and not take_all and run.stalled == 0:
            done, proven = eng.panel_run_spec(k, steps, take_all, run.spec_budget)
        else:
            done = proven = eng.panel_run(k, steps, take_all)
        tail = done > proven and done > 0
        if run.coop_check or (tail and spec_word is not None):      # the count stays on the device: min over ranks, ONE read
            if tail:
                eng.panel_project_spec_dev(k, done, proven, spec_word.data_ptr())
            else:
                spec_word.fill_(float(done))             # -1: failed here; otherwise the fully proven count
            comm.allreduce_min_tensor(spec_word)
            agreed = int(run.read_word())
            if agreed < 0:
                run.leave_kernel()
                continue
            if tail:
                done = agreed
        elif done < 0:            # one rank (tests): the context has switched the timed-out kernel off; repeat
            continue
        elif tail:
            mine = eng.panel_project_spec(k, done, proven)
            done = int(-comm.allreduce_max(np.array([-float(mine)]))[0]) if comm.multi else mine
        break
    if tail:                      # the pass has decided how much of the unproven tail stands
        eng.panel_commit(k, done)
        run.adapt_spec(done - proven)
    elif done > 0:                # all steps proven: the plain pass
        eng.panel_project(k, done)
    return done


def _refresh(run):
    """Nothing provable (stale bound / exact ties): exact energies everywhere, retry; a second failure forces the global
    first arg-max as the only candidate."""
    eng, comm = run.eng, run.comm
    run.stalled += 1
    if run.stalled > 3:
        raise ArithmeticError("deflation made no progress at component %d" % run.k)
    e, g = eng.panel_refresh(run.k)
    both = comm.allreduce_max(np.eye(comm.world)[comm.rank] * e) if comm.multi else np.array([e])
    gids = comm.all_gather_ints([g])[:, 0]
    order = sorted(range(comm.world), key=lambda r: (-both[r], gids[r]))
    run.forced_next = int(gids[order[0]])


def deflate_panels_multirank(eng, comm, n_rows, K):
    """Projection-mode deflation over several ranks.  Per PANEL (up to 16 components):
      1. every rank thresholds its OWN energies (two local histogram steps, no collective) and exports its ~768 largest
         energies + its local threshold; ONE small all-gather (12 KB per rank) gives every rank the same global
         threshold tau -- the (m_target+1)-th largest energy overall, never below a rank's local bound -- and the
         per-rank candidate counts;
      2. each rank rebuilds the exact residual rows of its own candidates (energy > tau); a padded all-gather of
         rows and of vertex ids replicates the ~768 candidate rows on every rank;
      3. every rank runs the identical greedy steps on them (no per-component collective), then projects its shard.
    Two collectives (energies; rows with their vertex ids packed behind them) and two host synchronisations per panel.
    Ranks stay in lock-step because every decision is a function of all-gathered data.
    Unproven steps (ASB_SPEC_PANELS, default on): when the bound on the vertices outside the candidate set is too stale
    to prove a winner, the panel goes on with the exact winner among the candidates (identical on every rank); the
    pass over X then checks those steps against every vertex's energy, each rank on its shard, and one extra tiny
    all-reduce (min) fixes how many of them stand -- fewer, longer panels for one more collective on such panels."""
    run = _Run(eng, comm, n_rows, K)
    while run.k < K:
        if run.guessing:
            eng.panel_guess_end()
            run.guessing = False
        if run.stall_rule and run.reads - run.mark_reads >= 8:           # (every quantity below is the same on all ranks)
            slow = (run.k - run.mark_k) * 4 < (run.reads - run.mark_reads) * 3
            run.mark_reads, run.mark_k = run.reads, run.k
            if slow:
                eng.project_switch_residual(run.k)
                _residual_rest(eng, comm, run.k, K)
                return run.k
        run.reads += 1
        forced = run.forced_next if run.stalled >= 2 else -1
        take_all = forced >= 0 or run.global_all
        done = 0
        if _candidates(run, forced, take_all):
            # one launch for several sub-panels where the kernel is on, nothing is forced or stalled and more than one
            # panel is left; one panel per read otherwise (also after the kernel timed out, and in the CPU test double)
            if run.multi_sub and run.spec_budget and not take_all and run.stalled == 0 and K - run.k > 16:
                done = _read_one_launch(run)
                if done is None:
                    continue                                  # the panel again, from the selection
            else:
                done = _read_plain(run, 1 if forced >= 0 else min(16, K - run.k), take_all)
        if done == 0:
            _refresh(run)
            continue
        run.stalled = 0
        run.k += done
    if run.guessing:
        eng.panel_guess_end()
    return K
