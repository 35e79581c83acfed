"""The model of the count-aware temporal accumulation (include/mipt.h "mipt_temporal_counts"), in numpy float32 over host arrays.
Written from the contract's text on top of temporal_model (its camera record, projection, history layout and comparisons): one rounded
f32 operation per operator, in the order written; a rejected tap is not added at all; a pixel without a sample does not read hdr.
Nothing comes from the library under test."""
import numpy as np

import temporal_model as TM

F = TM.F


def step(hdr, position, normal, depth, material, cameras, counts, samples_cap, history=None, albedo=None, alpha_min=0.0, max_history=32.0,
         normal_tol=0.1, depth_tol=0.1):
    """One call of mipt_temporal_counts.  As temporal_model.step, with `counts` [V,H,W] (or [H,W]) uint32 and the cap ->
    dict(out, history, length, variance, n, reuse, taps)."""
    hdr = np.asarray(hdr, dtype=F)
    single = hdr.ndim == 3
    hdr, position, normal, depth, albedo = (TM._lift(a, single) for a in (hdr, position, normal, depth, albedo))
    material = np.ascontiguousarray(material)
    material = TM._lift(material.view(np.uint32) if material.dtype.itemsize == 4 else material, single, np.uint32)
    counts = np.ascontiguousarray(counts)
    counts = TM._lift(counts.view(np.uint32) if counts.dtype.itemsize == 4 else counts, single, np.uint32)
    assert 1 <= samples_cap <= 65535
    v, h, w, _ = hdr.shape
    assert counts.shape == (v, h, w)
    cams = np.asarray(cameras).reshape(-1)
    assert len(cams) == v
    records = np.stack([TM.camera_record(c) for c in cams])
    alpha_min, max_history, normal_tol, depth_tol = F(alpha_min), F(max_history), F(normal_tol), F(depth_tol)
    n = np.minimum(counts, np.uint32(samples_cap))
    nf = n.astype(F)
    traced = n > 0
    with np.errstate(all="ignore"):
        a = np.where(albedo > TM.FLOOR, albedo, TM.FLOOR).astype(F) if albedo is not None else None
        src = np.where(traced[..., None], hdr, F(0.0)).astype(F)         # hdr is not read where n == 0
        cc = src / a if albedo is not None else src
        l = ((TM.LUMA[0] * cc[..., 0]) + (TM.LUMA[1] * cc[..., 1])) + (TM.LUMA[2] * cc[..., 2])
        ll = l * l
        zero = np.zeros((v, h, w), dtype=F)
        # RESET: n > 0 starts with nf samples (capped); n == 0 holds nothing
        c = np.where(traced[..., None], cc, F(0.0)).astype(F)
        length = np.where(traced, np.where(nf < max_history, nf, max_history), F(0.0)).astype(F)
        m1, m2 = np.where(traced, l, zero).astype(F), np.where(traced, ll, zero).astype(F)
        reuse_all = np.zeros((v, h, w), dtype=bool)
        taps_all = np.zeros((v, h, w), dtype=np.int32)
        if history is not None:
            rec, p0, p1, p2 = TM.unpack_history(history, v, h, w)
            for iv in range(v):
                hit = depth[iv] < TM.MISS
                d, vz, fx, fy, d2 = TM.project(position[iv], rec[iv], w, h)
                front = hit & (vz > F(0.0))
                inside = front & (fx >= F(-1.0)) & (fx < F(w)) & (fy >= F(-1.0)) & (fy < F(h))
                flx, fly = np.floor(np.where(inside, fx, F(0.0))), np.floor(np.where(inside, fy, F(0.0)))
                x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
                wx, wy = fx - flx, fy - fly
                ox, oy = F(1.0) - wx, F(1.0) - wy
                sw = np.zeros((h, w), dtype=F)
                s = np.zeros((h, w, 3), dtype=F)
                sl, s1, s2 = np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F), np.zeros((h, w), dtype=F)
                taps = np.zeros((h, w), dtype=np.int32)
                for qx, qy, wt in ((x0, y0, ox * oy), (x0 + 1, y0, wx * oy), (x0, y0 + 1, ox * wy), (x0 + 1, y0 + 1, wx * wy)):
                    in_frame = inside & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    sx_, sy_ = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    cq, gq, mq = p0[iv][sy_, sx_], p1[iv][sy_, sx_], p2[iv][sy_, sx_]
                    same_material = mq[..., 2] == material[iv]
                    dn = normal[iv] - gq[..., :3]
                    dn = ((dn[..., 0] * dn[..., 0]) + (dn[..., 1] * dn[..., 1])) + (dn[..., 2] * dn[..., 2])
                    normal_ok = dn <= normal_tol
                    depth_ok = np.abs(d2 - (gq[..., 3] * gq[..., 3])) <= depth_tol * d2
                    sampled = cq[..., 3] > F(0.0)                     # the new check: len_q > 0, a NaN rejected
                    ok = in_frame & same_material & normal_ok & depth_ok & sampled
                    sw = np.where(ok, sw + wt, sw)
                    s = np.where(ok[..., None], s + (wt[..., None] * cq[..., :3]), s)
                    sl = np.where(ok, sl + (wt * cq[..., 3]), sl)
                    s1 = np.where(ok, s1 + (wt * mq[..., 0].view(F)), s1)
                    s2 = np.where(ok, s2 + (wt * mq[..., 1].view(F)), s2)
                    taps += ok
                reuse = inside & (sw > TM.MIN_WEIGHT)
                safe = np.where(reuse, sw, F(1.0))
                cp, lp, q1, q2 = s / safe[..., None], sl / safe, s1 / safe, s2 / safe
                ln = lp + nf[iv]
                ln = np.where(ln < max_history, ln, max_history).astype(F)
                al = nf[iv] / ln
                al = np.where(al > alpha_min, al, alpha_min).astype(F)
                al = np.where(al < F(1.0), al, F(1.0)).astype(F)
                blend = reuse & traced[iv]
                keep = reuse & ~traced[iv]                            # pure reprojection
                c[iv] = np.where(blend[..., None], cp + ((cc[iv] - cp) * al[..., None]), np.where(keep[..., None], cp, c[iv]))
                m1[iv] = np.where(blend, q1 + ((l[iv] - q1) * al), np.where(keep, q1, m1[iv]))
                m2[iv] = np.where(blend, q2 + ((ll[iv] - q2) * al), np.where(keep, q2, m2[iv]))
                length[iv] = np.where(blend, ln, np.where(keep, np.where(lp < max_history, lp, max_history), length[iv]))
                reuse_all[iv], taps_all[iv] = reuse, taps
        out = (c * a if albedo is not None else c).astype(F)
        var = m2 - (m1 * m1)
        variance = np.where(var > F(0.0), var, F(0.0)).astype(F)
    hist = TM.pack_history(records, c, length, normal, depth, m1, m2, material)
    res = dict(out=out, history=hist, length=length, variance=variance, n=n, reuse=reuse_all, taps=taps_all)
    if single:
        res.update({k: res[k][0] for k in ("out", "length", "variance", "n", "reuse", "taps")})
    return res
