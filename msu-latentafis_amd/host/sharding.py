"""Gallery sharding and rank-list merge.  Pure host logic: numpy for the arithmetic, torch.distributed only for
the one exchange step (all_gather of the per-shard top-k; backend "nccl" = RCCL over xGMI on the GPU node, "gloo" in CPU tests).

Gallery templates are independent units: partition them into one contiguous shard per rank, balanced by the cost driver
(number of rolled texture points); every rank scores all queries against its shard and reports its local top-k with GLOBAL
gallery indices; the merged list is the top-k of the union in the lists' own order: rank_key(score) descending, ties by ascending global index.

The order is the one every path of the library lists by (csrc/rank_order.h, minu.hip::k_topk): rank_key is the ordered bits of score + 0.0f, so that the two
zeros are one value and a NaN stands where its bits put it (above +inf with the sign clear, below -inf with it set).  On NaN-free scores that is plainly score
descending.  The subject lists merge on subject_key, the ordered bits of the raw word (-0.0 below +0.0), the key include/afis_matcher.h documents for subjects.

A weighted search (Matcher.search_weighted) needs no merge of its own: the columns of shards are disjoint and the weights common to every rank, so the per-rank
lists read from its matrix are merge_hits / merge_subject_hits input as they are.

A print search (Matcher.search_prints) builds its queries from the resident shard, so a print is a query only on the rank that holds it.  Against the other
shards its template must be present there: the existing search_weighted route over host views of the print (n_wm = n_wt = 1) serves that, with the same bits.  Either
way the per-rank lists read from the matrix are merge_hits / merge_subject_hits input as they are.

A cascade search (Matcher.search_cascade) keeps per latent the `keep` best prints by the minutiae scorers alone: every rank keeps `keep` of its own shard.  The per-rank
lists read from its matrix are merge_hits / merge_subject_hits input as they are; their union contains the global stage-1 top `keep`, so the merged result is a
superset of the single-context cascade over the whole gallery, not the same list.  A print cascade (Matcher.search_prints_cascade) combines both rules: a print is a
query only on the rank that holds it, every rank keeps `keep` of its own shard, and the merged lists are a superset of the single-context result.  A cascade over a part
of the shard (Matcher.search_cascade_eligible, Matcher.search_cascade_subset) needs no new merge either: every rank keeps `keep` of its own shard's eligible (or listed)
prints, and the per-rank lists are merge_hits input as they are, a superset of the single-context result.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np


def _ordered(words: np.ndarray) -> np.ndarray:
    w = np.asarray(words, np.uint32)
    return np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000)).astype(np.uint32)


def rank_key(score) -> np.ndarray:
    """csrc/score_order.h::rank_key, stated in numpy: the uint32 key a template rank list is sorted on, descending."""
    return _ordered((np.asarray(score, np.float32) + np.float32(0.0)).view(np.uint32))


def subject_key(score) -> np.ndarray:
    """The key of the subject rank lists (subject_rank.hip): the ordered bits of the raw score word."""
    return _ordered(np.ascontiguousarray(score, np.float32).view(np.uint32))


def _desc(key: np.ndarray) -> np.ndarray:
    return -key.astype(np.int64)                                           # a lexsort column: key descending


def shard_bounds(cost: np.ndarray, world: int) -> List[Tuple[int, int]]:
    """Contiguous [lo, hi) per rank with ~equal total cost.  Every rank gets a (possibly empty) range; ranges tile [0, G)."""
    G = len(cost)
    if world <= 1:
        return [(0, G)]
    c = np.concatenate([[0], np.cumsum(np.asarray(cost, dtype=np.float64))])
    total = c[-1]
    cuts = [0]
    for r in range(1, world):
        target = total * r / world
        k = int(np.searchsorted(c, target, side="left"))
        k = min(max(k, cuts[-1]), G)
        cuts.append(k)
    cuts.append(G)
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def split_candidates(idx, bounds: List[Tuple[int, int]]) -> List[np.ndarray]:
    """A global candidate list over a shard plan (shard_bounds): per rank the indices that fall inside its [lo, hi) — its index_base and
    index_base + size — in the order the caller listed them, possibly none.  Each part is what that rank hands to Matcher.subset_create;
    the per-rank rank lists of the subset searches then merge with merge_topk / gather_topk as those of full searches do.
    An index outside every shard is an error (the ranges of a plan tile [0, G))."""
    a = np.asarray(idx, np.int64).reshape(-1)
    parts = [a[(a >= lo) & (a < hi)] for lo, hi in bounds]
    if sum(len(p) for p in parts) != len(a):
        covered = np.zeros(len(a), bool)
        for lo, hi in bounds:
            covered |= (a >= lo) & (a < hi)
        raise ValueError(f"split_candidates: indices outside the shard plan (or a plan whose ranges overlap): {a[~covered][:8].tolist()}")
    return parts


def merge_topk(idx: np.ndarray, score: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """idx, score: [R, Q, kk] per-shard rank lists (idx -1 = padding).  Returns the merged [Q, k] list: rank_key(score) descending, then global index ascending —
    whatever bits the scores hold, the first k of what one search over the union lists."""
    R, Q, kk = idx.shape
    fi = np.transpose(idx, (1, 0, 2)).reshape(Q, R * kk)
    fs = np.transpose(score, (1, 0, 2)).reshape(Q, R * kk).astype(np.float32)
    out_i = np.full((Q, k), -1, np.int64); out_s = np.full((Q, k), -np.inf, np.float32)
    for q in range(Q):
        valid = fi[q] >= 0
        vi, vs = fi[q][valid], fs[q][valid]
        order = np.lexsort((vi, _desc(rank_key(vs))))[:k]         # key descending, then global index ascending
        out_i[q, :len(order)] = vi[order]; out_s[q, :len(order)] = vs[order]
    return out_i, out_s


def merge_subject_topk(ids: np.ndarray, score: np.ndarray, best_idx: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """ids, score, best_idx: [R, Q, kk] per-rank subject rank lists (Matcher.rank_subjects on every rank's shard; id -1 = padding).  Returns the merged [Q, k] lists:
    entries with the same id keep the greater score — on equal scores the lower best_idx — then score descending, id ascending; padded with (-1, -inf, -1).
    "Greater", "equal" and "descending" are those of subject_key, the key the per-rank lists were made on: the raw bits in their total order, -0.0 below +0.0.

    Exact although a person's prints may lie in several shards, for kk >= k: a subject's global score is the maximum of its per-shard scores, reached in some shard A.
    If the subject is among the global k best, fewer than k subjects rank before it globally (greater score, or equal score and lower id); every subject that ranks
    before it INSIDE A does so with a per-shard score no greater than its own global one, hence ranks before it globally too — so it is among A's k best and arrives
    with its true score and best template (the lowest index at that score within A; the same score from another shard competes here on best_idx).  An entry that
    arrives only with a lower score — from shards where the subject did not reach its maximum, while A's list was full — belongs to a subject that k others outrank
    in A, all of them globally ahead of it: whatever place its understated score earns, it cannot be among the k best, and it cannot displace one of them, because
    each of those arrives with its true score."""
    R, Q, kk = ids.shape
    fi = np.transpose(ids, (1, 0, 2)).reshape(Q, R * kk)
    fs = np.transpose(score, (1, 0, 2)).reshape(Q, R * kk).astype(np.float32)
    fb = np.transpose(best_idx, (1, 0, 2)).reshape(Q, R * kk)
    out_i = np.full((Q, k), -1, np.int64); out_s = np.full((Q, k), -np.inf, np.float32); out_b = np.full((Q, k), -1, np.int64)
    for q in range(Q):
        valid = fi[q] >= 0
        vi, vs, vb = fi[q][valid], fs[q][valid], fb[q][valid]
        order = np.lexsort((vb, _desc(subject_key(vs)), vi))                # by id; inside an id the greater key, then the lower best_idx, comes first
        first = np.ones(len(order), bool); first[1:] = vi[order][1:] != vi[order][:-1]
        keep = order[first]
        vi, vs, vb = vi[keep], vs[keep], vb[keep]
        order = np.lexsort((vi, _desc(subject_key(vs))))[:k]                # key descending, then subject id ascending
        out_i[q, :len(order)] = vi[order]; out_s[q, :len(order)] = vs[order]; out_b[q, :len(order)] = vb[order]
    return out_i, out_s, out_b


def merge_hits(n_hits: np.ndarray, idx: np.ndarray, score: np.ndarray, cap: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """n_hits: [R, Q], idx, score: [R, Q, kk] per-rank hit lists (Matcher.rank_hits with one min_score on every rank's shard; kk >= cap).  Returns (n_hits [Q], idx [Q, cap],
    score [Q, cap]): the counts add — a template lies in one shard — and the list is merge_topk's (rank_key descending, then global index ascending), cut at cap.  Exact: every
    rank's list is the best-kk prefix of what qualifies in its shard, so an entry among the cap best of the union is among the kk best of its own shard.

    The column lists of a reverse search (Matcher.rank_latent_hits: Q = the prints searched, the entries are latents) merge by this same function when the LATENTS are
    split — over ranks, or over several query handles of one rank searched one after the other, each with its latent_base: the columns are common to every part, a
    latent lies in one part, so the counts add, and the list is the merge on score descending, then latent index ascending; exact for the reason above."""
    out_i, out_s = merge_topk(idx, score, cap)
    return np.asarray(n_hits, np.int64).sum(axis=0), out_i, out_s


def merge_prints_to_card(n_hits: np.ndarray, latent: np.ndarray, score: np.ndarray, cap: int):
    """n_hits: [P], latent, score: [P, kk] — the column lists of the P prints of ONE card (Matcher.rank_latent_hits with one min_score; row p = print position p;
    latent -1 = padding; kk >= cap).  Returns (latent [cap], score [cap], print_pos [cap], n_latents, truncated): per latent its greatest score over the card's prints — on
    equal scores the lowest print position — then score descending, latent index ascending, cut at cap and padded with (-1, -inf, -1).  print_pos says which print of
    the card the entry's score belongs to.  Scores compare on rank_key, the key of the column lists.

    Exact for kk >= cap: a latent's card score is the maximum of its per-print scores, reached at some print p.  If the latent is among the card's cap best, fewer than
    cap latents rank before it on the card (greater score, or equal score and lower index); every latent that ranks before it INSIDE p's list does so with a per-print
    score no greater than its own card score, hence ranks before it on the card too — so the latent is among the cap best of the print where it reaches its maximum and
    arrives with its true score.  An entry that arrives only with a lower score, from prints where the latent stays below its maximum while p's list was full, belongs
    to a latent that cap others outrank in p, all of them ahead of it on the card: it cannot be among the cap best and cannot displace one of them.
    The per-print counts do not add, for one latent may qualify against several prints of the card: n_latents is the number of distinct latents in the input.  That is
    the exact count while every print handed over all its hits; truncated is true when a print reported n_hits > kk, and only then is the count a lower bound
    (merge_subject_hits' rule)."""
    li = np.asarray(latent, np.int64)
    P, kk = li.shape
    fs = np.asarray(score, np.float32).reshape(P * kk)
    fp = np.repeat(np.arange(P, dtype=np.int64), kk)
    fl = li.reshape(P * kk)
    valid = fl >= 0
    vl, vs, vp = fl[valid], fs[valid], fp[valid]
    order = np.lexsort((vp, _desc(rank_key(vs)), vl))                       # by latent; inside a latent the greater key, then the lower print position, comes first
    first = np.ones(len(order), bool); first[1:] = vl[order][1:] != vl[order][:-1]
    keep = order[first]
    vl, vs, vp = vl[keep], vs[keep], vp[keep]
    order = np.lexsort((vl, _desc(rank_key(vs))))[:cap]                     # key descending, then latent index ascending
    out_l = np.full(cap, -1, np.int64); out_s = np.full(cap, -np.inf, np.float32); out_p = np.full(cap, -1, np.int64)
    out_l[:len(order)] = vl[order]; out_s[:len(order)] = vs[order]; out_p[:len(order)] = vp[order]
    return out_l, out_s, out_p, int(len(vl)), bool((np.asarray(n_hits, np.int64) > kk).any())


def merge_subject_hits(n_hits: np.ndarray, subject: np.ndarray, score: np.ndarray, best_idx: np.ndarray, cap: int):
    """n_hits: [R, Q], subject, score, best_idx: [R, Q, kk] per-rank subject hit lists (Matcher.rank_subject_hits with one min_score on every rank; kk >= cap).  Returns
    (n_hits [Q], truncated [Q], subject, score, best_idx [Q, cap]).  The lists merge by merge_subject_topk's rule — a person's prints may lie in several shards: the best
    score wins, then the lowest index — which is exact for the same reason (a subject's global score is its best per-shard score, and it qualifies where it reaches that).
    The per-rank counts do NOT add, for the same person may qualify in several shards: n_hits[q] is the number of distinct subjects in the merged input.  That is the exact
    count while every rank handed over all its hits; truncated[q] is true when a rank reported n_hits > kk, and only then is the count a lower bound."""
    ids = np.asarray(subject)
    R, Q, kk = ids.shape
    out = merge_subject_topk(ids, score, best_idx, cap)
    flat = np.transpose(ids, (1, 0, 2)).reshape(Q, R * kk)
    n = np.array([len(np.unique(row[row >= 0])) for row in flat], np.int64)
    return n, (np.asarray(n_hits, np.int64) > kk).any(axis=0), out[0], out[1], out[2]


def merge_case_subject_hits(n_hits: np.ndarray, subject: np.ndarray, score: np.ndarray, cap: int, mode: int):
    """n_hits: [R, C], subject, score: [R, C, kk] per-rank case subject lists (Matcher.rank_case_subject_hits with one case_of, mode and min_score on every rank; kk >= cap;
    subject -1 = padding).  Returns (n_hits [C], truncated [C], subject [C, cap], score [C, cap]), on rank_key, the key of the case lists.  (The TEMPLATE lists of the cases
    need no function of their own: the columns of different shards are disjoint and a case's row is common to every rank, so they merge with merge_hits as they are.)

    mode 1 (AFIS_CASE_MAX): exact although a person's prints may lie in several shards.  The fused value is a maximum over the members of a maximum over the subject's
    templates, and maxima commute: it is the greatest of the per-rank fused values.  Entries with the same id keep the greater key, then the list is key descending,
    id ascending — merge_subject_hits' argument: a subject among the cap best arrives from the rank where it reaches its value, with that value.  The per-rank counts do
    not add; n_hits is the number of distinct subjects in the input, exact unless a rank was cut (truncated: a rank reported n_hits > kk).
    mode 0 (AFIS_CASE_SUM): exact only while no subject's prints lie in two shards.  Rank r holds sum_m max_{t in r} s(m, t), and the sum over the members of the maxima
    over ALL of a subject's templates is in general neither the greatest nor the sum of those.  With whole subjects per shard every id arrives from one rank, the counts
    add and the lists merge as template lists do; an id that two ranks report raises ValueError."""
    ids = np.asarray(subject, np.int64)
    R, C, kk = ids.shape
    if mode not in (0, 1):
        raise ValueError(f"merge_case_subject_hits: mode {mode} is neither 0 (AFIS_CASE_SUM) nor 1 (AFIS_CASE_MAX)")
    fi = np.transpose(ids, (1, 0, 2)).reshape(C, R * kk)
    fs = np.transpose(np.asarray(score, np.float32), (1, 0, 2)).reshape(C, R * kk)
    counts = np.asarray(n_hits, np.int64)
    out_n = np.empty(C, np.int64); out_i = np.full((C, cap), -1, np.int64); out_s = np.full((C, cap), -np.inf, np.float32)
    for c in range(C):
        valid = fi[c] >= 0
        vi, vs = fi[c][valid], fs[c][valid]
        if mode == 0:
            u, n = np.unique(vi, return_counts=True)
            if (n > 1).any():
                raise ValueError(f"merge_case_subject_hits: AFIS_CASE_SUM lists merge only while every subject's prints lie in one shard; ids {u[n > 1][:8].tolist()} arrive from two ranks")
            out_n[c] = counts[:, c].sum()
        else:
            order = np.lexsort((_desc(rank_key(vs)), vi))                   # by id; inside an id the greater key comes first
            first = np.ones(len(order), bool); first[1:] = vi[order][1:] != vi[order][:-1]
            vi, vs = vi[order[first]], vs[order[first]]
            out_n[c] = len(vi)
        order = np.lexsort((vi, _desc(rank_key(vs))))[:cap]                 # key descending, then subject id ascending
        out_i[c, :len(order)] = vi[order]; out_s[c, :len(order)] = vs[order]
    return out_n, (counts > kk).any(axis=0), out_i, out_s


POS_LISTED, POS_NO_ENTRY, POS_NOT_COVERED = 0, 1, 2                         # AFIS_POS_* (include/afis_matcher.h)


def merge_positions(status: np.ndarray, score: np.ndarray, n_before_per_rank: np.ndarray):
    """Global rank positions of one target list handed to every rank.  status, score: [R, T] from Matcher.rank_positions on every rank (the columns of different shards
    are disjoint, so at most one rank covers a target: the OWNER, the rank whose status is not AFIS_POS_NOT_COVERED); n_before_per_rank: [R, T] from Matcher.count_before
    on every rank with the owner's score and the target's global index — every rank counts the entries of its own columns that stand before the target, the owner leaving
    the target's own column out.  Returns (status [T], score [T], n_before [T], owner [T]): the owner's status and score; n_before the sum of the counts over the ranks
    where the owner lists the target, else -1; owner -1, status AFIS_POS_NOT_COVERED, score -inf, n_before -1 for a target no rank covers.  Two ranks covering one
    target raise ValueError: their columns are not disjoint."""
    st = np.asarray(status, np.int32); sc = np.asarray(score, np.float32); nb = np.asarray(n_before_per_rank, np.int64)
    if st.ndim != 2 or sc.shape != st.shape or nb.shape != st.shape:
        raise ValueError("merge_positions: status, score and n_before_per_rank are [ranks, targets] arrays of one shape")
    covered = st != POS_NOT_COVERED
    if (covered.sum(axis=0) > 1).any():
        raise ValueError(f"merge_positions: targets {np.flatnonzero(covered.sum(axis=0) > 1)[:8].tolist()} are covered by two ranks")
    T = st.shape[1]
    any_owner = covered.any(axis=0)
    owner = np.where(any_owner, covered.argmax(axis=0) if st.shape[0] else 0, -1).astype(np.int64)
    at = (np.maximum(owner, 0), np.arange(T))
    out_status = np.where(any_owner, st[at] if st.shape[0] else POS_NOT_COVERED, POS_NOT_COVERED).astype(np.int32)
    out_score = np.full(T, -np.inf, np.float32)
    if st.shape[0]:
        out_score[any_owner] = sc[at][any_owner]                            # (own bits: a masked copy, no arithmetic)
    n_before = np.where(out_status == POS_LISTED, nb.sum(axis=0), -1).astype(np.int64)
    return out_status, out_score, n_before, owner


# afis_score_stat (include/afis_matcher.h), 48 bytes: Matcher.score_stats' rows
SCORE_STAT = np.dtype([("n", "<i8"), ("n_outside", "<i8"), ("s1", "<u8"), ("s2_lo", "<u8"), ("s2_hi", "<u8"), ("min", "<f4"), ("max", "<f4")])
STAT_MAX_CELLS = 1 << 27                                                    # the bound of csrc/score_stats.h: n <= 2^27, for a shard and for a sum of shards
_M64 = (1 << 64) - 1


def _valued(score: np.float32) -> bool:
    """csrc/score_stats.h::stat_cell_class == valued, for a score that is not the no-entry word: finite, the sign of score + 0 clear, below 2^16."""
    s = np.float32(score)
    return bool(np.isfinite(s) and not np.signbit(s + np.float32(0.0)) and s < np.float32(65536.0) and s.view(np.uint32) != np.uint32(0xffffffff))


def merge_score_stats(per_rank) -> np.ndarray:
    """Statistics of disjoint shards added up.  per_rank: [R, rows] SCORE_STAT — Matcher.score_stats(axis=0) of every rank for one query list (or, along axis 1,
    of disjoint latent files against one print list).  -> [rows]: n, n_outside, s1 and the 128-bit s2 added in Python integers, min of mins and max of maxes over the
    ranks that hold a valued cell (+inf / -inf where none does): what one context over the whole gallery returns, bit for bit, wherever the shards were cut.
    ValueError where a row's n would pass 2^27."""
    a = np.asarray(per_rank, SCORE_STAT)
    if a.ndim != 2:
        raise ValueError("merge_score_stats: per_rank is a [ranks, rows] array of SCORE_STAT")
    out = np.zeros(a.shape[1], SCORE_STAT)
    out["min"] = np.inf; out["max"] = -np.inf
    for i in range(a.shape[1]):
        n = n_out = s1 = s2 = 0
        lo, hi = np.float32(np.inf), np.float32(-np.inf)
        for r in range(a.shape[0]):
            e = a[r, i]
            n += int(e["n"]); n_out += int(e["n_outside"]); s1 += int(e["s1"]); s2 += (int(e["s2_hi"]) << 64) | int(e["s2_lo"])
            if int(e["n"]) > 0:
                lo = e["min"] if rank_key(e["min"]) < rank_key(lo) else lo
                hi = e["max"] if rank_key(e["max"]) > rank_key(hi) else hi
        if n > STAT_MAX_CELLS:
            raise ValueError(f"merge_score_stats: row {i} would hold {n} valued cells, a statistic takes 2^27")
        out[i] = (n, n_out, s1, s2 & _M64, s2 >> 64, lo, hi)
    return out


def trim_score_stats(stats, top_scores) -> np.ndarray:
    """A cohort without its best cells: from row i of stats [rows] the valued scores of top_scores[i] (a sequence per row: the row's merged top-k, say) are taken out
    exactly, as afis_score_stat_remove takes them — n - 1, s1 - q, s2 - q^2 with q = rint(float64(score) x 2^20).  Scores that are not valued (a list's -inf padding,
    -1) are skipped: they were never in n.  min and max stay as they are.  ValueError where a field would go below zero: the score was not in the cohort."""
    st = np.asarray(stats, SCORE_STAT).reshape(-1).copy()
    if len(top_scores) != len(st):
        raise ValueError("trim_score_stats: one sequence of scores per row")
    for i in range(len(st)):
        n, s1, s2 = int(st[i]["n"]), int(st[i]["s1"]), (int(st[i]["s2_hi"]) << 64) | int(st[i]["s2_lo"])
        for s in np.asarray(top_scores[i], np.float32).reshape(-1):
            if not _valued(s):
                continue
            q = int(np.rint(np.float64(s) * 1048576.0))
            n -= 1; s1 -= q; s2 -= q * q
            if n < 0 or s1 < 0 or s2 < 0:
                raise ValueError(f"trim_score_stats: row {i} does not hold the score {float(s)!r}")
        st[i]["n"] = n; st[i]["s1"] = s1; st[i]["s2_lo"] = s2 & _M64; st[i]["s2_hi"] = s2 >> 64
    return st


def merge_score_histograms(per_rank) -> np.ndarray:
    """Histograms of disjoint shards added up.  per_rank: [R, rows, bins] int64 — Matcher.score_histogram(edges, axis=0) of every rank for one query list and ONE list
    of edges (or, along axis 1, of disjoint latent files against one print list).  -> [rows, bins] int64, a plain integer sum: what one context over the whole gallery
    returns, bit for bit, wherever the shards were cut.  ValueError where the ranks' shapes differ or a count is negative."""
    parts = [np.asarray(p) for p in per_rank]
    if not parts or any(p.ndim != 2 or p.shape != parts[0].shape or p.dtype.kind not in "iu" for p in parts):
        raise ValueError("merge_score_histograms: per_rank is [ranks, rows, bins] integer counts, every rank with the same edges")
    a = np.stack([p.astype(np.int64) for p in parts])
    if (a < 0).any():
        raise ValueError("merge_score_histograms: a count is negative")
    return a.sum(axis=0, dtype=np.int64)


def _person_aligned(who: str, ids_per_rank):
    """The ranks' id lists as int64 arrays; ValueError where an id appears in two of them."""
    ids = [np.asarray(i, np.int64).reshape(-1) for i in ids_per_rank]
    if not ids:
        raise ValueError(f"{who}: no rank")
    every = np.concatenate(ids)
    u, n = np.unique(every, return_counts=True)
    if (n > 1).any():
        raise ValueError(f"{who}: person distributions merge only for galleries sharded by person — a person's best score is a maximum over ALL their prints, and "
                         f"maxima of two ranks neither add nor concatenate; ids {u[n > 1][:8].tolist()} appear in two ranks' lists")
    return ids, every


def _merge_subject_rows(who: str, per_rank, ids_per_rank, axis: int, add):
    if axis not in (0, 1):
        raise ValueError(f"{who}: axis {axis} is neither 0 (queries) nor 1 (subjects)")
    ids, every = _person_aligned(who, ids_per_rank)
    parts = list(per_rank)
    if len(parts) != len(ids):
        raise ValueError(f"{who}: one id list per rank")
    if axis == 0:
        return add(parts)
    if any(len(p) != len(i) for p, i in zip(parts, ids)):
        raise ValueError(f"{who}: along axis 1 a rank returns one row per id of its list")
    order = np.argsort(every, kind="stable")
    return every[order], np.concatenate([np.asarray(p) for p in parts])[order]


def merge_subject_score_stats(per_rank, ids_per_rank, axis: int):
    """Person statistics of the ranks of a gallery SHARDED BY PERSON.  per_rank: every rank's Matcher.subject_score_stats(handle, axis) for one query list;
    ids_per_rank: every rank's distinct subject ids (handle[2]).  ValueError where an id appears in two ranks' lists: that person's prints straddle two shards, each rank
    holds the maximum over its own share, and neither the sum nor either value is the person's cell (merge_case_subject_hits' AFIS_CASE_SUM caveat).  axis 0: the
    ranks hold disjoint persons of one query's cohort, so the statistics add -> merge_score_stats' [n_q].  axis 1: every person lies on one rank ->
    (ids ascending, rows): the ranks' rows concatenated in id order."""
    return _merge_subject_rows("merge_subject_score_stats", per_rank, ids_per_rank, axis, merge_score_stats)


def merge_subject_score_histograms(per_rank, ids_per_rank, axis: int):
    """merge_subject_score_stats for Matcher.subject_score_histogram(handle, edges, axis) with ONE list of edges on every rank: axis 0 adds through
    merge_score_histograms -> [n_q, bins]; axis 1 -> (ids ascending, [subjects, bins]).  ValueError where an id appears in two ranks' lists."""
    return _merge_subject_rows("merge_subject_score_histograms", per_rank, ids_per_rank, axis, merge_score_histograms)


def histogram_rank_bin(counts, rank):
    """Where a rank falls in a histogram: counts [rows, bins] (or [bins]) int64 — merged, for a global rank — and rank [rows] (or a number) >= 0, counted from the
    best entry as afis_entries_at counts.  -> (bin, residual): the bin that holds the entry at that rank when the bins are walked from the top, and the rank among
    that bin's entries — the entries of all higher bins stand before it; (-1, rank) where the rank is not below the row's total.  With edges e, the entry's score
    lies in [e[bin - 1], e[bin]): the bracket INTEGRATION.md's sharded quantile recipe settles with afis_count_before."""
    c = np.asarray(counts, np.int64); one = c.ndim == 1
    c = c.reshape(1, -1) if one else c
    r = np.asarray(rank, np.int64).reshape(-1)
    if c.ndim != 2 or c.shape[1] == 0 or len(r) not in (1, c.shape[0]) or (c < 0).any() or (r < 0).any():
        raise ValueError("histogram_rank_bin: counts is [rows, bins] (or [bins]) of counts >= 0, rank one number >= 0 per row")
    r = np.broadcast_to(r, (c.shape[0],))
    above = np.cumsum(c[:, ::-1], axis=1)[:, ::-1]                          # above[i, b]: the entries of bins b .. of row i
    inside = above > r[:, None]                                             # bins b whose tail holds the rank: 0 .. the bin we want
    b = inside.sum(axis=1) - 1
    ok = b >= 0
    higher = np.where(ok, np.take_along_axis(above, np.maximum(b, 0)[:, None], axis=1)[:, 0] - np.take_along_axis(c, np.maximum(b, 0)[:, None], axis=1)[:, 0], 0)
    res = np.where(ok, r - higher, r).astype(np.int64)
    b = np.where(ok, b, -1).astype(np.int64)
    return (int(b[0]), int(res[0])) if one else (b, res)


def merge_link_groups(per_rank):
    """Link groups of the ranks of a sharded gallery merged by member name: per_rank is what Matcher.link_groups / link_subject_groups returned on every rank — a sequence
    of {"group_off": [g + 1], "member": [group_off[-1]]}, every rank's lists complete (n_listed == n_groups) —; groups of different ranks that share a member become one
    group (a host union over the names).  Named nodes share one name space across ranks: global template indices, or subject ids.  The anonymous rows -1 - q are shared
    only when every rank ran the SAME queries, the usual sharded latent search; otherwise rename them before merging.  -> {"n_groups", "n_members", "group_off",
    "member"} in the calls' own order: members by ascending name, then the anonymous rows by ascending q; groups by their first member.  With AFIS_LINK_ANY that is
    what one context over the whole gallery returns.  AFIS_LINK_MUTUAL groups merge correctly only where a pair's two cells lie on one rank: a rank confirms a cell
    by a reverse cell of its own matrix, so a pair of prints enrolled on two ranks is confirmed by neither.  ValueError where a CSR is malformed."""
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for r in per_rank:
        off = np.asarray(r["group_off"], np.int64).reshape(-1); mem = np.asarray(r["member"], np.int64).reshape(-1)
        if len(off) < 1 or off[0] != 0 or (np.diff(off) < 2).any() or off[-1] != len(mem):
            raise ValueError("merge_link_groups: group_off is a CSR into member, from 0 to len(member), every group of two or more")
        for g in range(len(off) - 1):
            names = [int(t) for t in mem[off[g]:off[g + 1]]]
            for t in names:
                parent.setdefault(t, t)
            a = find(names[0])
            for t in names[1:]:
                b = find(t)
                if a != b:
                    parent[b] = a
    key = lambda t: (0, t) if t >= 0 else (1, -1 - t)                       # named nodes by name, then the anonymous rows by q
    groups = {}
    for t in parent:
        groups.setdefault(find(t), []).append(t)
    out = sorted((sorted(g, key=key) for g in groups.values()), key=lambda g: key(g[0]))
    off = np.zeros(len(out) + 1, np.int64)
    off[1:] = np.cumsum([len(g) for g in out])
    member = np.array([t for g in out for t in g], np.int64)
    return {"n_groups": len(out), "n_members": len(member), "group_off": off, "member": member}


CORR_NOT_RUN, CORR_NOT_COVERED = -1, -2                                    # AFIS_CORR_* (include/afis_matcher.h)
PAIR_OK, PAIR_NOT_COVERED = 0, 1                                            # AFIS_PAIR_* (include/afis_matcher.h)


def merge_correspondences(per_rank_counts, per_rank_xy, per_rank_part=None):
    """One pair list handed to every rank of a sharded gallery (Matcher.correspondences_pairs' raw arrays): per_rank_counts [R, P, 3], per_rank_xy [R, P, 3, 120, 4],
    per_rank_part [R, P, 3] or None.  The shards' templates are disjoint, so at most one rank covers a pair — the rank whose counts are not AFIS_CORR_NOT_COVERED —
    and the pair is taken from it, bytes as they are.  Returns (counts [P, 3], xy [P, 3, 120, 4], owner [P]) — with per_rank_part also part [P, 3], before owner — :
    counts AFIS_CORR_NOT_COVERED, xy and part zero, owner -1 for a pair no rank covers.  Two ranks covering one pair raise ValueError."""
    cn = np.asarray(per_rank_counts, np.int32); xy = np.asarray(per_rank_xy, np.int16)
    if cn.ndim != 3 or cn.shape[2] != 3 or xy.shape != cn.shape + (120, 4):
        raise ValueError("merge_correspondences: counts is [ranks, pairs, 3] and xy [ranks, pairs, 3, 120, 4]")
    pt = None if per_rank_part is None else np.asarray(per_rank_part, np.float32)
    if pt is not None and pt.shape != cn.shape:
        raise ValueError("merge_correspondences: part is [ranks, pairs, 3], as counts")
    covered = (cn != CORR_NOT_COVERED).any(axis=2)                          # (a rank answers a pair with three times -2 or not at all)
    if (covered.sum(axis=0) > 1).any():
        raise ValueError(f"merge_correspondences: pairs {np.flatnonzero(covered.sum(axis=0) > 1)[:8].tolist()} are covered by two ranks")
    P = cn.shape[1]
    any_owner = covered.any(axis=0) if cn.shape[0] else np.zeros(P, bool)
    owner = np.where(any_owner, covered.argmax(axis=0) if cn.shape[0] else 0, -1).astype(np.int64)
    out_c = np.full((P, 3), CORR_NOT_COVERED, np.int32); out_xy = np.zeros((P, 3, 120, 4), np.int16); out_p = np.zeros((P, 3), np.float32)
    have = np.flatnonzero(any_owner)
    out_c[have] = cn[owner[have], have]; out_xy[have] = xy[owner[have], have]
    if pt is not None:
        out_p[have] = pt[owner[have], have]
    return (out_c, out_xy, owner) if pt is None else (out_c, out_xy, out_p, owner)


def merge_pair_scores(per_rank):
    """One pair list handed to every rank of a sharded gallery: per_rank is what Matcher.score_pairs returned on every rank, a sequence of {"status": [P], "score": [P],
    "parts": [P, 4] or None}.  The shards' templates are disjoint, so at most one rank covers a pair — the rank whose status is AFIS_PAIR_OK — and the pair is taken from
    it, bits as they are.  Returns {"status", "score", "parts" (None unless every rank gave parts), "owner": [P] the covering rank}: a pair no rank covers stays
    AFIS_PAIR_NOT_COVERED / -inf / +0.0 with owner -1.  Two ranks covering one pair raise ValueError."""
    per_rank = list(per_rank)
    st = np.asarray([np.asarray(r["status"], np.int32).reshape(-1) for r in per_rank], np.int32).reshape(len(per_rank), -1)
    sc = np.asarray([np.asarray(r["score"], np.float32).reshape(-1) for r in per_rank], np.float32).reshape(len(per_rank), -1)
    if st.shape != sc.shape:
        raise ValueError("merge_pair_scores: status and score are [pairs] on every rank, of one length")
    P = st.shape[1]
    with_parts = len(per_rank) > 0 and all(r.get("parts") is not None for r in per_rank)
    pt = np.asarray([np.asarray(r["parts"], np.float32).reshape(-1, 4) for r in per_rank], np.float32).reshape(len(per_rank), -1, 4) if with_parts else None
    if pt is not None and pt.shape != st.shape + (4,):
        raise ValueError("merge_pair_scores: parts is [pairs, 4] on every rank")
    covered = st == PAIR_OK
    if (covered.sum(axis=0) > 1).any():
        raise ValueError(f"merge_pair_scores: pairs {np.flatnonzero(covered.sum(axis=0) > 1)[:8].tolist()} are covered by two ranks")
    any_owner = covered.any(axis=0) if st.shape[0] else np.zeros(P, bool)
    owner = np.where(any_owner, covered.argmax(axis=0) if st.shape[0] else 0, -1).astype(np.int64)
    out_st = np.full(P, PAIR_NOT_COVERED, np.int32); out_sc = np.full(P, -np.inf, np.float32); out_p = np.zeros((P, 4), np.float32) if with_parts else None
    have = np.flatnonzero(any_owner)
    out_st[have] = st[owner[have], have]; out_sc[have] = sc[owner[have], have]
    if with_parts:
        out_p[have] = pt[owner[have], have]
    return {"status": out_st, "score": out_sc, "parts": out_p, "owner": owner}


def merge_print_pair_scores(per_rank):
    """merge_pair_scores for Matcher.score_print_pairs' answers: per_rank a sequence of {"status": [P], "score": [P], "parts": [P, 2] or None}, one pair list handed to
    every rank.  A pair is covered by the one rank that holds BOTH prints and taken from it, bits as they are; a pair whose prints lie in two shards is covered by no
    rank and stays AFIS_PAIR_NOT_COVERED / -inf / +0.0 with owner -1.  Returns {"status", "score", "parts" [P, 2] (None unless every rank gave parts), "owner": [P]}.
    Two ranks covering one pair raise ValueError."""
    per_rank = list(per_rank)
    R = len(per_rank)
    st = np.asarray([np.asarray(r["status"], np.int32).reshape(-1) for r in per_rank], np.int32).reshape(R, -1)
    sc = np.asarray([np.asarray(r["score"], np.float32).reshape(-1) for r in per_rank], np.float32).reshape(R, -1)
    if st.shape != sc.shape:
        raise ValueError("merge_print_pair_scores: status and score are [pairs] on every rank, of one length")
    P = st.shape[1]
    with_parts = R > 0 and all(r.get("parts") is not None for r in per_rank)
    pt = np.asarray([np.asarray(r["parts"], np.float32).reshape(-1, 2) for r in per_rank], np.float32).reshape(R, -1, 2) if with_parts else None
    if pt is not None and pt.shape != st.shape + (2,):
        raise ValueError("merge_print_pair_scores: parts is [pairs, 2] on every rank")
    covered = st == PAIR_OK
    if (covered.sum(axis=0) > 1).any():
        raise ValueError(f"merge_print_pair_scores: pairs {np.flatnonzero(covered.sum(axis=0) > 1)[:8].tolist()} are covered by two ranks")
    any_owner = covered.any(axis=0) if R else np.zeros(P, bool)
    owner = np.where(any_owner, covered.argmax(axis=0) if R else 0, -1).astype(np.int64)
    out_st = np.full(P, PAIR_NOT_COVERED, np.int32); out_sc = np.full(P, -np.inf, np.float32); out_p = np.zeros((P, 2), np.float32) if with_parts else None
    have = np.flatnonzero(any_owner)
    out_st[have] = st[owner[have], have]; out_sc[have] = sc[owner[have], have]
    if with_parts:
        out_p[have] = pt[owner[have], have]
    return {"status": out_st, "score": out_sc, "parts": out_p, "owner": owner}


def merge_print_correspondences(per_rank_counts, per_rank_xy, per_rank_part=None):
    """merge_correspondences for Matcher.correspondences_print_pairs' raw arrays: per_rank_counts [R, P], per_rank_xy [R, P, 120, 4], per_rank_part [R, P] or None.  The
    rank whose count is not AFIS_CORR_NOT_COVERED holds both prints of the pair and the pair is taken from it, bytes as they are.  Returns (counts [P], xy [P, 120, 4],
    owner [P]) — with per_rank_part also part [P], before owner —: counts AFIS_CORR_NOT_COVERED, xy and part zero, owner -1 for a pair no rank covers (its prints lie in
    two shards, or in none).  Two ranks covering one pair raise ValueError."""
    cn = np.asarray(per_rank_counts, np.int32); xy = np.asarray(per_rank_xy, np.int16)
    if cn.ndim != 2 or xy.shape != cn.shape + (120, 4):
        raise ValueError("merge_print_correspondences: counts is [ranks, pairs] and xy [ranks, pairs, 120, 4]")
    pt = None if per_rank_part is None else np.asarray(per_rank_part, np.float32)
    if pt is not None and pt.shape != cn.shape:
        raise ValueError("merge_print_correspondences: part is [ranks, pairs], as counts")
    covered = cn != CORR_NOT_COVERED
    if (covered.sum(axis=0) > 1).any():
        raise ValueError(f"merge_print_correspondences: pairs {np.flatnonzero(covered.sum(axis=0) > 1)[:8].tolist()} are covered by two ranks")
    P = cn.shape[1]
    any_owner = covered.any(axis=0) if cn.shape[0] else np.zeros(P, bool)
    owner = np.where(any_owner, covered.argmax(axis=0) if cn.shape[0] else 0, -1).astype(np.int64)
    out_c = np.full(P, CORR_NOT_COVERED, np.int32); out_xy = np.zeros((P, 120, 4), np.int16); out_p = np.zeros(P, np.float32)
    have = np.flatnonzero(any_owner)
    out_c[have] = cn[owner[have], have]; out_xy[have] = xy[owner[have], have]
    if pt is not None:
        out_p[have] = pt[owner[have], have]
    return (out_c, out_xy, owner) if pt is None else (out_c, out_xy, out_p, owner)


def gather_topk(idx: np.ndarray, score: np.ndarray, k: int, device=None, force: bool = False):
    """The one exchange step: all_gather of [Q, kk] (int64 idx, f32 score) from every rank, then merge on every rank.
    Messages are tiny (24 x 12 B per query per rank); this is latency-, not bandwidth-bound."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size() == 1 and not force):
        return merge_topk(idx[None], score[None], k)
    world = dist.get_world_size()
    dev = device if device is not None else "cpu"
    ti = torch.from_numpy(np.ascontiguousarray(idx)).to(dev)
    ts = torch.from_numpy(np.ascontiguousarray(score)).to(dev)
    gi = [torch.empty_like(ti) for _ in range(world)]
    gs = [torch.empty_like(ts) for _ in range(world)]
    dist.all_gather(gi, ti)
    dist.all_gather(gs, ts)
    ai = torch.stack(gi).cpu().numpy(); as_ = torch.stack(gs).cpu().numpy()
    return merge_topk(ai, as_, k)


class CppExchange:
    """The exchange step of the C++ `match` host (csrc/rank_exchange.cpp: ncclAllGather over RCCL / xGMI on a dedicated HIP stream, staged
    through device buffers; AFIS_EXCHANGE=tcp swaps in the TCP stand-in that lets ranks share a GPU), bound with ctypes from
    libafis_exchange.so.  Ranks and rendezvous come from RANK / WORLD_SIZE / LOCAL_RANK / MASTER_ADDR / MASTER_PORT (the id exchange uses
    MASTER_PORT + 1, IPv4 literal only).  No fallback: a missing library raises."""

    def __init__(self, device: int):
        import ctypes as C
        import os
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", "libafis_exchange.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: build it with `make -C msu-latentafis_amd/csrc`")
        self._C = C
        lib = self.lib = C.CDLL(path)
        lib.afis_exchange_create.restype = C.c_void_p; lib.afis_exchange_create.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        lib.afis_exchange_all_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        lib.afis_exchange_last_error.restype = C.c_char_p; lib.afis_exchange_last_error.argtypes = [C.c_void_p]
        lib.afis_exchange_destroy.restype = None; lib.afis_exchange_destroy.argtypes = [C.c_void_p]
        for f in ("afis_exchange_world", "afis_exchange_rank", "afis_exchange_is_rccl", "afis_exchange_comm_count", "afis_exchange_comm_device"):
            getattr(lib, f).argtypes = [C.c_void_p]
        err = C.create_string_buffer(512)
        self.h = lib.afis_exchange_create(device, err, 512)
        if not self.h:
            raise RuntimeError("afis_exchange_create: " + err.value.decode(errors="replace"))
        self.world = lib.afis_exchange_world(self.h); self.rank = lib.afis_exchange_rank(self.h)
        self.is_rccl = bool(lib.afis_exchange_is_rccl(self.h))
        self.comm_count = int(lib.afis_exchange_comm_count(self.h))         # ncclCommCount of this rank's communicator (-1: the TCP stand-in has none)
        self.comm_device = int(lib.afis_exchange_comm_device(self.h))       # ncclCommCuDevice

    def all_gather(self, block: np.ndarray) -> np.ndarray:
        """block: any contiguous array, the same shape and dtype on every rank -> [world, *block.shape]."""
        b = np.ascontiguousarray(block)
        out = np.empty((self.world,) + b.shape, b.dtype)
        rc = self.lib.afis_exchange_all_gather(self.h, b.ctypes.data, out.ctypes.data, b.nbytes)
        if rc != 0:
            raise RuntimeError("afis_exchange_all_gather: " + self.lib.afis_exchange_last_error(self.h).decode(errors="replace"))
        return out

    def gather_topk(self, idx: np.ndarray, score: np.ndarray, k: int):
        """One all-gather of the per-rank block [Q][kk] x (idx i64, score f32), as `match -l` sends it, then the merge."""
        Q, kk = idx.shape
        blk = np.empty(Q * kk * 12, np.uint8)
        blk[:Q * kk * 8] = np.ascontiguousarray(idx, np.int64).view(np.uint8).ravel()
        blk[Q * kk * 8:] = np.ascontiguousarray(score, np.float32).view(np.uint8).ravel()
        allb = self.all_gather(blk)
        ai = allb[:, :Q * kk * 8].copy().view(np.int64).reshape(self.world, Q, kk)
        as_ = allb[:, Q * kk * 8:].copy().view(np.float32).reshape(self.world, Q, kk)
        return merge_topk(ai, as_, k)

    def close(self):
        if self.h:
            self.lib.afis_exchange_destroy(self.h); self.h = None


CORR_MOMENTS = np.dtype([(f, "<i8") for f in ("n", "slx", "sly", "srx", "sry", "dot", "cross", "ll", "rr")])   # afis_corr_moments (include/afis_matcher.h), 72 bytes


def _one_owner(who, covered):
    """covered [R, P] -> (any_owner [P] bool, owner [P] int64, -1 where no rank covers); two ranks covering one pair raise ValueError."""
    R, P = covered.shape
    if (covered.sum(axis=0) > 1).any():
        raise ValueError(f"{who}: pairs {np.flatnonzero(covered.sum(axis=0) > 1)[:8].tolist()} are covered by two ranks")
    any_owner = covered.any(axis=0) if R else np.zeros(P, bool)
    return any_owner, np.where(any_owner, covered.argmax(axis=0) if R else 0, -1).astype(np.int64)


def merge_texture_correspondences(per_rank):
    """One pair list handed to every rank of a sharded gallery: per_rank is what Matcher.texture_correspondences_pairs (or its print form) returned on every rank, a
    sequence of {"counts": [P], "xy": [P, 200, 4], "pt": [P, 200, 2], "sim": [P, 200], "part": [P] or None}.  At most one rank covers a pair — the rank whose count is
    not AFIS_CORR_NOT_COVERED — and the pair is taken from it, bytes as they are, as merge_correspondences does.  Returns {"counts", "xy", "pt", "sim", "part" (None
    unless every rank gave it), "owner": [P]}: counts AFIS_CORR_NOT_COVERED, everything else zero and owner -1 for a pair no rank covers.  Two ranks covering one pair
    raise ValueError."""
    per_rank = list(per_rank)
    R = len(per_rank)
    cn = np.asarray([np.asarray(r["counts"], np.int32).reshape(-1) for r in per_rank], np.int32).reshape(R, -1)
    P = cn.shape[1]
    xy = np.asarray([np.asarray(r["xy"], np.int16).reshape(-1, 200, 4) for r in per_rank], np.int16).reshape(R, -1, 200, 4)
    pt = np.asarray([np.asarray(r["pt"], np.int16).reshape(-1, 200, 2) for r in per_rank], np.int16).reshape(R, -1, 200, 2)
    sim = np.asarray([np.asarray(r["sim"], np.float32).reshape(-1, 200) for r in per_rank], np.float32).reshape(R, -1, 200)
    if xy.shape[:2] != cn.shape or pt.shape[:2] != cn.shape or sim.shape[:2] != cn.shape:
        raise ValueError("merge_texture_correspondences: counts is [pairs], xy [pairs, 200, 4], pt [pairs, 200, 2] and sim [pairs, 200] on every rank, of one length")
    with_part = R > 0 and all(r.get("part") is not None for r in per_rank)
    part = np.asarray([np.asarray(r["part"], np.float32).reshape(-1) for r in per_rank], np.float32).reshape(R, -1) if with_part else None
    if part is not None and part.shape != cn.shape:
        raise ValueError("merge_texture_correspondences: part is [pairs] on every rank")
    any_owner, owner = _one_owner("merge_texture_correspondences", cn != CORR_NOT_COVERED)
    out = {"counts": np.full(P, CORR_NOT_COVERED, np.int32), "xy": np.zeros((P, 200, 4), np.int16), "pt": np.zeros((P, 200, 2), np.int16), "sim": np.zeros((P, 200), np.float32),
           "part": np.zeros(P, np.float32) if with_part else None, "owner": owner}
    have = np.flatnonzero(any_owner)
    out["counts"][have] = cn[owner[have], have]; out["xy"][have] = xy[owner[have], have]; out["pt"][have] = pt[owner[have], have]; out["sim"][have] = sim[owner[have], have]
    if with_part:
        out["part"][have] = part[owner[have], have]
    return out


def merge_pair_alignments(per_rank):
    """One pair list handed to every rank: per_rank is what Matcher.pair_alignments (or print_pair_alignments) returned on every rank, a sequence of {"status": [P],
    "moments": [P, K] CORR_MOMENTS} (K = 4, or 2 for print pairs).  The rank whose status is AFIS_PAIR_OK covers the pair and its records are taken, bytes as they are.
    Returns {"status", "moments", "owner": [P]}: AFIS_PAIR_NOT_COVERED, zero records and owner -1 for a pair no rank covers.  Two ranks covering one pair raise
    ValueError."""
    per_rank = list(per_rank)
    R = len(per_rank)
    st = np.asarray([np.asarray(r["status"], np.int32).reshape(-1) for r in per_rank], np.int32).reshape(R, -1)
    P = st.shape[1]
    moms = [np.asarray(r["moments"], CORR_MOMENTS) for r in per_rank]
    K = moms[0].shape[-1] if R and moms[0].ndim == 2 else 4
    if any(m.shape != (P, K) for m in moms):
        raise ValueError("merge_pair_alignments: moments is [pairs, 4] (or [pairs, 2]) on every rank, one row per status entry")
    any_owner, owner = _one_owner("merge_pair_alignments", st == PAIR_OK)
    out_st = np.full(P, PAIR_NOT_COVERED, np.int32); out_m = np.zeros((P, K), CORR_MOMENTS)
    have = np.flatnonzero(any_owner)
    if len(have):
        mo = np.stack(moms)
        out_st[have] = st[owner[have], have]; out_m[have] = mo[owner[have], have]
    return {"status": out_st, "moments": out_m, "owner": owner}
