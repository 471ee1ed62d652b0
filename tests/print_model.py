"""Numpy model of the print search (afis_search_prints), shared by tests/test_prints_host.py and tests/test_gpu_print_search.py: the query view of a resident print
(its minutiae template as held; its texture points clamped to 1000 with the PQ codes decoded through the codebook), the decode itself, the query-side tables and
arrays of one launch group — the destination CSRs, the descriptor fragment tiles — and the plan (activity, one pseudo-query per print, the fold's tables, batches)."""
import importlib

import numpy as np

import weighted_model as W

T = importlib.import_module("msu-latentafis_amd.host.templates")

TEX_MAX = 1000                                                              # kTexMax: the clamp at enrolment
TILE_ROWS, TILE16_ROWS, FRAG_ROWS = 8, 16, 16


def decode(words, codes):
    """des[r][6 m + k] = words[m][codes[r][m]][k]: the bits copied.  words [16][256][6] float32, codes [n][16] uint8 -> [n][96] float32"""
    words = np.asarray(words, np.float32); codes = np.asarray(codes, np.uint8).reshape(-1, words.shape[0])
    m = np.arange(words.shape[0])
    return np.ascontiguousarray(words[m[None, :], codes.astype(np.int64)].reshape(len(codes), -1))


def resident(print_):
    """What the shard holds of a print: (minutiae template or None, texture template clamped to 1000 points or None)."""
    mt = print_.minu[0] if len(print_.minu) and print_.minu[0].n > 0 else None
    tt = None
    if len(print_.tex) and print_.tex[0].n > 0:
        x = print_.tex[0]; n = min(x.n, TEX_MAX)
        tt = T.TextureTemplate(np.asarray(x.x[:n], np.int16), np.asarray(x.y[:n], np.int16), np.asarray(x.ori[:n], np.float32), codes=np.asarray(x.codes[:n], np.uint8))
    return mt, tt


def view(print_, words):
    """The query view P of a resident print: n_minu = 1 with the template as held, n_tex = 1 with the resident points and the decoded descriptors."""
    mt, tt = resident(print_)
    out = T.FPTemplate()
    if mt is not None:
        out.minu.append(T.MinutiaeTemplate(np.asarray(mt.x, np.int16), np.asarray(mt.y, np.int16), np.asarray(mt.ori, np.float32), np.asarray(mt.des, np.float32)))
    if tt is not None:
        out.tex.append(T.TextureTemplate(tt.x, tt.y, tt.ori, des=decode(words, tt.codes)))
    return out


def view_bytes(v):
    """Bytes the view's arrays hold: what the route over host views uploads for it."""
    return sum(m.n * (8 + 4 * 96) for m in v.minu) + sum(t.n * (8 + 4 * 96) for t in v.tex)


def fragment_tiles(des):
    """[n][96] -> [ceil(n / 16)][6][64][4]: lane l, component c of load v holds des[16 tile + (l & 15)][4 (4 v + c) + (l >> 4)]; rows past the end are zero."""
    des = np.asarray(des, np.float32).reshape(-1, 96)
    n_tiles = (len(des) + FRAG_ROWS - 1) // FRAG_ROWS
    pad = np.zeros((n_tiles * FRAG_ROWS, 96), np.float32); pad[:len(des)] = des
    out = np.zeros((n_tiles, 6, 64, 4), np.float32)
    lane = np.arange(64)
    for v in range(6):
        for c in range(4):
            col = 4 * (4 * v + c) + (lane >> 4)
            out[:, v, :, c] = pad.reshape(n_tiles, FRAG_ROWS, 96)[:, lane & 15, col]
    return out


def group(prints, words, use_minu=None, use_tex=None):
    """One launch group whose queries are `prints`: the seven tables and the seven arrays, as build_group makes them for the views under the selection
    (0 or -1, -1, -1, 0 or -1).  -> dict of arrays named as QueryDev's members."""
    n = len(prints)
    use_minu = np.ones(n, bool) if use_minu is None else np.asarray(use_minu, bool)
    use_tex = np.ones(n, bool) if use_tex is None else np.asarray(use_tex, bool)
    lm_off, lm_tile_off, lt_off, tile_off, tile16_off, tex_slot = [0], [0], [0], [0], [0], []
    lm_xy, lm_ori, lm_des, lm_frag, lt_xy, lt_ori, lt_des = [], [], [], [], [], [], []
    lt_max = 0
    for p, pr in enumerate(prints):
        mt, tt = resident(pr)
        nm = mt.n if (mt is not None and use_minu[p]) else 0
        nt = tt.n if (tt is not None and use_tex[p]) else 0
        if nm:
            lm_xy.append(np.stack([mt.x, mt.y], 1).astype(np.int16)); lm_ori.append(np.asarray(mt.ori, np.float32)); lm_des.append(np.asarray(mt.des, np.float32))
            lm_frag.append(fragment_tiles(mt.des))
        if nt:
            lt_xy.append(np.stack([tt.x, tt.y], 1).astype(np.int16)); lt_ori.append(tt.ori); lt_des.append(decode(words, tt.codes))
        lm_off += [lm_off[-1] + nm] * 3                                     # slot 0 holds the template, slots 1 and 2 are empty ranges
        lm_tile_off += [lm_tile_off[-1] + (nm + FRAG_ROWS - 1) // FRAG_ROWS] * 3
        lt_off.append(lt_off[-1] + nt)
        tile_off.append(tile_off[-1] + (nt + TILE_ROWS - 1) // TILE_ROWS)
        tile16_off.append(tile16_off[-1] + (nt + TILE16_ROWS - 1) // TILE16_ROWS)
        tex_slot.append((1 if mt is not None else 0) if nt else -1)
        lt_max = max(lt_max, nt)

    def cat(parts, shape, dtype):
        return np.concatenate(parts).astype(dtype) if parts else np.zeros(shape, dtype)
    i32 = lambda a: np.array(a, np.int32)
    return {"lm_off": i32(lm_off), "lm_tile_off": i32(lm_tile_off), "lt_off": i32(lt_off), "tile_off": i32(tile_off), "tile16_off": i32(tile16_off),
            "tex_slot": i32(tex_slot), "status": np.zeros(n, np.int32),
            "lm_xy": cat(lm_xy, (0, 2), np.int16), "lm_ori": cat(lm_ori, (0,), np.float32), "lm_des": cat(lm_des, (0, 96), np.float32),
            "lm_frag": cat(lm_frag, (0, 6, 64, 4), np.float32), "lt_xy": cat(lt_xy, (0, 2), np.int16), "lt_ori": cat(lt_ori, (0,), np.float32),
            "lt_des": cat(lt_des, (0, 96), np.float32), "lt_pad": max(TILE_ROWS, (lt_max + TILE_ROWS - 1) // TILE_ROWS * TILE_ROWS)}


def plan(prints, w_minu, w_tex):
    """-> (qd [n_q][4] int32 = (first pseudo-query, n_pq in {0, 1}, n_at, status), use [P][2] bool = (minutiae, texture) of every pseudo-query, wtab [P][4] float32):
    afis_search_weighted's plan for the views with n_wm = n_wt = 1."""
    counts = [(int(resident(p)[0] is not None), int(resident(p)[1] is not None)) for p in prints]
    wm = np.asarray(w_minu, np.float32).reshape(-1, 1); wt = np.asarray(w_tex, np.float32).reshape(-1, 1)
    qd, spec, wtab = W.plan(counts, wm, wt)
    assert ((spec[:, 1:3] == -1).all() and np.isin(spec[:, [0, 3]], (0, -1)).all()) if len(spec) else True
    return qd, (spec[:, [0, 3]] == 0) if len(spec) else np.zeros((0, 2), bool), wtab


def h2d_bytes(qd, cap, groups_of=lambda n: [n]):
    """Bytes afis_search_prints hands to host-to-device copies: per launch group of n pseudo-queries ten tables padded to 16 bytes, per batch the fold's 16 bytes per
    query and per pseudo-query.  groups_of(n) -> the sizes of the launch groups a batch of n pseudo-queries is cut into."""
    pad4 = lambda k: (k + 3) // 4 * 4
    total = 0
    for q0, q1 in W.batches(qd, cap):
        n_p = int(qd[q0:q1, 1].sum())
        total += (q1 - q0) * 16 + n_p * 16
        for n in (groups_of(n_p) if n_p else []):
            total += 4 * (2 * pad4(3 * n + 1) + 3 * pad4(n + 1) + 5 * pad4(n))
    return total
