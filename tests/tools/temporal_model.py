"""The model of the temporal accumulation (include/mipt.h "temporal accumulation"), in numpy float32 over host arrays.  Written from
the contract's text: one rounded f32 operation per operator, in the order written; the camera record is formed in Python floats
(binary64); a rejected tap is not added at all.  Nothing comes from the library under test.

A history is a flat uint32 array of 16*V + 12*N words (N = V*H*W): the layout the header documents.  Besides the outputs the model
returns a class code per pixel and the reasons its taps were rejected, so that the tests can assert that their inputs reach every
branch."""
import numpy as np

F = np.float32
FLOOR = F(1.0 / 256.0)
MIN_WEIGHT = F(1.0 / 64.0)
MISS = F(1e30)
LUMA = (F(0.2126), F(0.7152), F(0.0722))
DEFAULTS = dict(alpha_min=0.0, max_history=32.0, normal_tol=0.1, depth_tol=0.1)

# the camera of the frame before, relative to the scene's (position offset, degrees of pitch and yaw): on the 20 k-triangle atrium at
# 64x36 this move puts pixels of the next frame, taken from the scene's camera, into every class below (asserted by the tests)
COVERAGE_MOVE = dict(dp=(0.3, 0.1, 0.2), dpitch=2.0, dyaw=40.0)

# class codes
FIRST, MISSED, BEHIND, OFF_FRAME, THIN, REUSED4, REUSED3, REUSED2, REUSED1 = range(9)
CLASS_NAMES = ("first frame", "miss", "behind the camera", "off frame", "sw too small", "reused with 4 taps", "reused with 3 taps",
               "reused with 2 taps", "reused with 1 tap")
# bits of `rejects`: a tap inside the frame failed this check (the checks run in this order; a tap counts for the first it fails)
REJ_MATERIAL, REJ_NORMAL, REJ_DEPTH = 1, 2, 4
REJECT_NAMES = {REJ_MATERIAL: "taps rejected by material", REJ_NORMAL: "taps rejected by normal", REJ_DEPTH: "taps rejected by depth"}


def camera_record(camera):
    """One CAMERA record -> the 16 f32 of its history record (B row-major, C, four zeros), or None if it has no inverse"""
    look_at = np.asarray(camera["look_at"], dtype=F).reshape(4, 4)
    a = [[float(look_at[c][r]) for c in range(3)] for r in range(3)]
    k = [[0.0] * 3 for _ in range(3)]
    k[0][0] = (a[1][1] * a[2][2]) - (a[1][2] * a[2][1])
    k[0][1] = (a[1][2] * a[2][0]) - (a[1][0] * a[2][2])
    k[0][2] = (a[1][0] * a[2][1]) - (a[1][1] * a[2][0])
    k[1][0] = (a[0][2] * a[2][1]) - (a[0][1] * a[2][2])
    k[1][1] = (a[0][0] * a[2][2]) - (a[0][2] * a[2][0])
    k[1][2] = (a[0][1] * a[2][0]) - (a[0][0] * a[2][1])
    k[2][0] = (a[0][1] * a[1][2]) - (a[0][2] * a[1][1])
    k[2][1] = (a[0][2] * a[1][0]) - (a[0][0] * a[1][2])
    k[2][2] = (a[0][0] * a[1][1]) - (a[0][1] * a[1][0])
    det = ((a[0][0] * k[0][0]) + (a[0][1] * k[0][1])) + (a[0][2] * k[0][2])
    if det == 0.0 or not np.isfinite(det):
        return None
    rec = np.zeros(16, dtype=F)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                rec[i * 3 + j] = F(k[j][i] / det)
    if not np.isfinite(rec[:9]).all():
        return None
    rec[9:12] = np.asarray(camera["position"], dtype=F).reshape(3)
    return rec


def history_words(v, h, w):
    return 16 * v + 12 * v * h * w


def unpack_history(history, v, h, w):
    """flat uint32 history -> (records [V,16] f32, plane0 [V,H,W,4] f32, plane1 [V,H,W,4] f32, plane2 [V,H,W,4] u32): views, not copies"""
    hist = np.ascontiguousarray(history).reshape(-1).view(np.uint32)
    n = v * h * w
    assert hist.size == history_words(v, h, w)
    rec = hist[: 16 * v].view(F).reshape(v, 16)
    planes = hist[16 * v:].reshape(3, n * 4)
    return rec, planes[0].view(F).reshape(v, h, w, 4), planes[1].view(F).reshape(v, h, w, 4), planes[2].reshape(v, h, w, 4)


def pack_history(records, colour, length, normal, depth, m1, m2, material):
    """the planes of [V,H,W(,3)] -> a flat uint32 history"""
    v, h, w = length.shape
    hist = np.zeros(history_words(v, h, w), dtype=np.uint32)
    rec, p0, p1, p2 = unpack_history(hist, v, h, w)
    rec[:] = records
    p0[..., :3], p0[..., 3] = colour, length
    p1[..., :3], p1[..., 3] = normal, depth
    p2[..., 0], p2[..., 1], p2[..., 2] = np.asarray(m1, dtype=F).view(np.uint32), np.asarray(m2, dtype=F).view(np.uint32), material
    return hist


def _lift(a, single, dtype=F):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=dtype)
    return a[None] if single else a


def project(position, record, w, h):
    """d = position - C, the camera-space vector v and the pixel coordinates (fx, fy) of the contract, all f32 -> (d, vz, fx, fy, d2)"""
    with np.errstate(all="ignore"):
        B, Cc = record[:9].reshape(3, 3), record[9:12]
        d = position - Cc
        vv = [((B[i][0] * d[..., 0]) + (B[i][1] * d[..., 1])) + (B[i][2] * d[..., 2]) for i in range(3)]
        sx, sy = -(vv[0] / vv[2]), vv[1] / vv[2]
        wf, hf = F(w), F(h)
        aspect = wf / hf
        fx = (((sx / aspect) + F(1.0)) * F(0.5)) * wf
        fy = hf - (((sy + F(1.0)) * F(0.5)) * hf)
        d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
    return d, vv[2], fx, fy, d2


def step(hdr, position, normal, depth, material, cameras, history=None, albedo=None, alpha_min=0.0, max_history=32.0, normal_tol=0.1,
         depth_tol=0.1):
    """One call of mipt_temporal.  hdr [V,H,W,3] (or [H,W,3]) and the guides of the same leading shape, `cameras` V CAMERA records,
    `history` the flat uint32 history of the previous frame or None -> dict(out, history, length, variance, cls, rejects)."""
    hdr = np.asarray(hdr, dtype=F)
    single = hdr.ndim == 3
    hdr, position, normal, depth, albedo = (_lift(a, single) for a in (hdr, position, normal, depth, albedo))
    material = np.ascontiguousarray(material)
    material = _lift(material.view(np.uint32) if material.dtype.itemsize == 4 else material, single, np.uint32)   # int32 tensors hold the same bits
    v, h, w, _ = hdr.shape
    cams = np.asarray(cameras).reshape(-1)
    assert len(cams) == v
    records = np.stack([camera_record(c) for c in cams])
    alpha_min, max_history, normal_tol, depth_tol = F(alpha_min), F(max_history), F(normal_tol), F(depth_tol)
    with np.errstate(all="ignore"):
        if albedo is not None:
            a = np.where(albedo > FLOOR, albedo, FLOOR).astype(F)       # a NaN albedo gives the floor
            cc = hdr / a
        else:
            cc = hdr
        l = ((LUMA[0] * cc[..., 0]) + (LUMA[1] * cc[..., 1])) + (LUMA[2] * cc[..., 2])
        ll = l * l
        c, length, m1, m2 = cc.copy(), np.ones((v, h, w), dtype=F), l.copy(), ll.copy()          # RESET
        cls = np.full((v, h, w), FIRST, dtype=np.int32)
        rejects = np.zeros((v, h, w), dtype=np.int32)
        if history is not None:
            rec, p0, p1, p2 = unpack_history(history, v, h, w)
            for iv in range(v):
                hit = depth[iv] < MISS
                d, vz, fx, fy, d2 = project(position[iv], rec[iv], w, h)
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
                    rejects[iv] |= np.where(in_frame & ~same_material, REJ_MATERIAL, 0)
                    rejects[iv] |= np.where(in_frame & same_material & ~normal_ok, REJ_NORMAL, 0)
                    rejects[iv] |= np.where(in_frame & same_material & normal_ok & ~depth_ok, REJ_DEPTH, 0)
                    ok = in_frame & same_material & normal_ok & depth_ok
                    sw = np.where(ok, sw + wt, sw)
                    s = np.where(ok[..., None], s + (wt[..., None] * cq[..., :3]), s)
                    sl = np.where(ok, sl + (wt * cq[..., 3]), sl)
                    s1 = np.where(ok, s1 + (wt * mq[..., 0].view(F)), s1)
                    s2 = np.where(ok, s2 + (wt * mq[..., 1].view(F)), s2)
                    taps += ok
                reuse = inside & (sw > MIN_WEIGHT)
                safe = np.where(reuse, sw, F(1.0))
                cp, lp, q1, q2 = s / safe[..., None], sl / safe, s1 / safe, s2 / safe
                ln = lp + F(1.0)
                ln = np.where(ln < max_history, ln, max_history).astype(F)
                al = F(1.0) / ln
                al = np.where(al > alpha_min, al, alpha_min).astype(F)
                c[iv] = np.where(reuse[..., None], cp + ((cc[iv] - cp) * al[..., None]), cc[iv])
                m1[iv] = np.where(reuse, q1 + ((l[iv] - q1) * al), l[iv])
                m2[iv] = np.where(reuse, q2 + ((ll[iv] - q2) * al), ll[iv])
                length[iv] = np.where(reuse, ln, F(1.0))
                cls[iv] = np.where(~hit, MISSED, np.where(~front, BEHIND, np.where(~inside, OFF_FRAME, np.where(~reuse, THIN, REUSED4 + 4 - taps))))
        out = (c * a if albedo is not None else c).astype(F)
        var = m2 - (m1 * m1)
        variance = np.where(var > F(0.0), var, F(0.0)).astype(F)
    hist = pack_history(records, c, length, normal, depth, m1, m2, material)
    res = dict(out=out, history=hist, length=length, variance=variance, cls=cls, rejects=rejects)
    if single:
        res.update({k: res[k][0] for k in ("out", "length", "variance", "cls", "rejects")})
    return res


def classes_present(results):
    """the names of every class and rejection reason that occurs in these step() results"""
    seen = set()
    for r in results:
        seen.update(CLASS_NAMES[int(k)] for k in np.unique(r["cls"]))
        bits = int(np.bitwise_or.reduce(r["rejects"].reshape(-1))) if r["rejects"].size else 0
        seen.update(name for bit, name in REJECT_NAMES.items() if bits & bit)
    return seen


ALL_CLASSES = set(CLASS_NAMES) | set(REJECT_NAMES.values())


def same_bits(a, b):
    """bit for bit on uint32 views, a NaN equal to any NaN (its sign and payload are the implementation's)"""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def same_history(a, b, v, h, w):
    """every byte of two histories: the float words as same_bits, the material and padding words exactly"""
    ra, a0, a1, a2 = unpack_history(a, v, h, w)
    rb, b0, b1, b2 = unpack_history(b, v, h, w)
    return (same_bits(ra, rb) and same_bits(a0, b0) and same_bits(a1, b1) and same_bits(a2[..., :2].view(F), b2[..., :2].view(F))
            and bool(np.array_equal(a2[..., 2:], b2[..., 2:])))


def rmse(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.sqrt(np.mean(d * d)))
