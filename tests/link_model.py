"""The numpy / plain Python model of the link groups (include/afis_matcher.h: afis_link_groups, afis_link_subject_groups), shared by tests/test_link_groups_host.py and
tests/test_gpu_link_groups.py.  Never the code under test: a cell's key is ordered((x + 0).view(u32)) as in tests/test_gpu_score_hist.py's model, a cell reaches when
its key >= the key of min_score (which is >= the key of -inf: the no-entry word never reaches), the filter is that file's label test and exclusion lists, the edges
are spelled out cell by cell under both modes and both forms, the components come from a dictionary union-find and the CSR from sorted Python lists.

Names: a column's node is its name — a global template index, or the subject id of its template —, row q's node is row_node[q] when that is >= 0 and the anonymous
name -1 - q otherwise.  Output order: named nodes by ascending name, then anonymous rows by ascending q; groups by their first member."""
import numpy as np

FLOOR = 0x007fffff                                                          # the key of -inf
ANY, MUTUAL = 0, 1
U64 = np.uint64


def ordered(words):
    w = np.asarray(words, np.uint32)
    return np.where(w & np.uint32(0x80000000), ~w, w | np.uint32(0x80000000)).astype(np.uint32)


def key_of(x):
    with np.errstate(invalid="ignore"):
        return ordered((np.asarray(x, np.float32) + np.float32(0.0)).view(np.uint32))


def label_test(labels, masks):
    L = np.asarray(labels, U64)[None, :]; mk = np.asarray(masks, U64)
    a, b, c = mk[:, 0:1], mk[:, 1:2], mk[:, 2:3]
    return ((a == 0) | ((L & a) != 0)) & ((L & b) == b) & ((L & c) == 0)


def not_excluded(names, excl, n_q):
    """ok [n_q][columns]: column c is not on row q's list; names [columns] the names the list is written in (global indices, or the columns' subject ids)."""
    ok = np.ones((n_q, len(names)), bool)
    for q in range(n_q):
        ok[q] = ~np.isin(names, np.asarray(excl[q], np.int64))
    return ok


def reach_matrix(scores, min_score, ok=None):
    """[n_q][columns] bool: the cell is an entry the filter leaves and reaches min_score."""
    thr = int(key_of(np.float32(min_score)))
    assert thr >= FLOOR
    r = key_of(scores) >= thr
    return r if ok is None else r & ok


def node_key(t):
    return (0, t) if t >= 0 else (1, -1 - t)


def edges(reach, col_name, row_node, mode, glob=None):
    """The cells that are edges, as (row node name, column node name) per cell.  reach [n_q][C] bool in any column order; col_name [C] the node name of every column;
    row_node [n_q] or None; glob [C]: the columns' global template indices (only where col_name is not that: the subject form's "first column of a person")."""
    n_q, C = reach.shape
    col_name = np.asarray(col_name, np.int64)
    glob = col_name if glob is None else np.asarray(glob, np.int64)
    rn = np.full(n_q, -1, np.int64) if row_node is None else np.asarray(row_node, np.int64)
    rname = [int(rn[q]) if rn[q] >= 0 else -1 - q for q in range(n_q)]
    first_row = {}
    for q in range(n_q):
        first_row.setdefault(rname[q], q)
    first_col = {}                                                          # the column of a row's print: the column of that name; for a person the first by global index
    for c in np.argsort(glob, kind="stable"):
        first_col.setdefault(int(col_name[c]), int(c))
    out = []
    for q, c in zip(*np.nonzero(reach)):
        a, b = rname[q], int(col_name[c])
        if a == b:
            continue
        if mode == MUTUAL:
            r2, c2 = first_row.get(b), first_col.get(a)
            if r2 is None or c2 is None or not reach[r2, c2]:
                continue
        out.append((a, b))
    return out


def components(edge_list):
    parent = {}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edge_list:
        parent.setdefault(a, a); parent.setdefault(b, b)
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[rb] = ra
    groups = {}
    for t in parent:
        groups.setdefault(find(t), []).append(t)
    return sorted((sorted(g, key=node_key) for g in groups.values()), key=lambda g: node_key(g[0]))


def csr(groups, cap_groups=None, cap_members=None):
    """-> n_groups, n_members, n_listed, group_off [n_listed + 1], member: the longest prefix of the groups that fits both caps (None: no cap)."""
    n_members = sum(len(g) for g in groups)
    off, member = [0], []
    for g in groups:
        if (cap_groups is not None and len(off) - 1 >= cap_groups) or (cap_members is not None and len(member) + len(g) > cap_members):
            break
        member += g; off.append(len(member))
    return len(groups), n_members, len(off) - 1, np.array(off, np.int64), np.array(member, np.int64)


def link(scores, min_score, col_name, row_node=None, mode=ANY, ok=None, glob=None, cap_groups=None, cap_members=None):
    """What the calls return, as Matcher.link_groups' dictionary."""
    e = edges(reach_matrix(scores, min_score, ok), col_name, row_node, mode, glob)
    n_groups, n_members, n_listed, off, member = csr(components(e), cap_groups, cap_members)
    return {"n_edges": len(e), "n_groups": n_groups, "n_members": n_members, "n_listed": n_listed, "group_off": off, "member": member}
