"""Plain reference of Detect with Fast NMS (csrc/detect.hip) that exposes what every stage hands to the next, and the known-answer
cases of tests/test_detect_kat_host.py (CPU) and tests/test_gpu_detect_kat.py (MI355X).

Semantics: layers/functions/detection.py:81-180 (Detect.detect, fast_nms, cc_fast_nms) and layers/box_utils.py:33-80, 304-310
of the reference, as oracle/yolact_oracle.py:260-316 cites them, but written independently of the oracle: numpy, explicit loops
over images and classes, a stable argsort over the kept priors in index order (so equal scores go to the lowest index; nothing
of torch).  The stages are the kernels' own:

  k1  softmax (float64, rounded) + foreground max / argmax + keep, class-major scores whose sign bit is set where keep == 0
  k2  per (image, class): the top_k kept priors by (score desc, index asc), decode, Fast NMS; all top_k slots, -1 where nothing
  k3  per image: the best `cap` survivors by (score desc, flat index asc: class-major, rank-minor), gathered outputs + record

Decode and IoU run in np.float32, one operation per statement, in the order of csrc/detect_common.h decode_box and of
iou_col_suppressed's comment: ((area_i + area_j) - inter), IoU = inter / union, keep = max <= thresh (False for NaN).  exp is the
one library function in there: by default the correctly rounded one (float64, rounded once); a caller that compares with torch
passes torch's (`exp32`).  The same quantities are computed in float64 for the margins a case reports.

Perturbed variants (keyword `variant`, only to prove that a case has teeth): 'ties_high', 'lt', 'conf_ge', 'rcp', 'nan_zero'.
"""
import numpy as np

F = np.float32
NT = 1024
SORT_N = 256
C_MAX = 234          # 64 * C * 4 <= 60000: the LDS check of ymi_detect_f32
VARIANTS = ('ties_high', 'lt', 'conf_ge', 'rcp', 'nan_zero')


def nxt(x):
    return np.nextafter(F(x), F(np.inf))


def prv(x):
    return np.nextafter(F(x), F(-np.inf))


def exp32_rounded(x):
    return np.exp(x.astype(np.float64)).astype(F)


# ---- K1 ----------------------------------------------------------------------------------------------------------------------------

def softmax64(rows):
    z = rows.astype(np.float64)
    z = z - z.max(-1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(-1, keepdims=True)


def k1(conf, C, ld, is_logits, conf_thresh, variant=None):
    """conf [B,P,ld] float32 (ld >= C: the first C entries of a row are real) -> dict(keep, num_keep, maxsc, argmax, scores_t
    [B,C-1,P], scores64 [B,P,C] (the float64 softmax, or conf itself), min_conf_margin = min |maxsc - conf_thresh|)."""
    conf = np.asarray(conf, F)
    B, P = conf.shape[:2]
    assert conf.shape[2] == ld >= C
    real = conf[:, :, :C]
    s64 = softmax64(real) if is_logits else real.astype(np.float64)
    s = s64.astype(F)
    th = F(conf_thresh)
    keep = np.zeros((B, P), np.int32)
    maxsc = np.zeros((B, P), F)
    argmax = np.zeros((B, P), np.int32)
    for b in range(B):
        fg = s[b, :, 1:]
        argmax[b] = np.argmax(fg, 1)                      # the first index wins a tie; background-excluded: class c -> c - 1
        maxsc[b] = fg[np.arange(P), argmax[b]]
        keep[b] = (maxsc[b] >= th) if variant == 'conf_ge' else (maxsc[b] > th)
    scores_t = np.ascontiguousarray(s[:, :, 1:].transpose(0, 2, 1))
    bits = scores_t.view(np.uint32).copy()
    bits[np.broadcast_to(keep[:, None, :] == 0, bits.shape)] |= np.uint32(0x80000000)
    return dict(keep=keep, num_keep=keep.sum(1).astype(np.int32), maxsc=maxsc, argmax=argmax, scores_t=bits.view(F),
                scores64=s64, min_conf_margin=float(np.abs(maxsc.astype(np.float64) - float(th)).min()))


# ---- decode / IoU ------------------------------------------------------------------------------------------------------------------

def decode32(loc, pr, exp32=exp32_rounded):
    """[n,4], [n,4] float32 -> [n,4]: c = p.xy + (loc.xy * 0.1) * p.wh; s = p.wh * exp(loc.wh * 0.2); xy1 = c - s / 2; xy2 = s + xy1."""
    out = np.empty((len(loc), 4), F)
    with np.errstate(all='ignore'):
        for a in range(2):
            t = loc[:, a] * F(0.1)
            t = t * pr[:, 2 + a]
            c = pr[:, a] + t
            e = loc[:, 2 + a] * F(0.2)
            e = exp32(e)
            s = pr[:, 2 + a] * e
            h = s / F(2)
            lo = c - h
            out[:, a] = lo
            out[:, 2 + a] = s + lo
    assert out.dtype == F
    return out


def decode64(loc, pr):
    loc, pr = loc.astype(np.float64), pr.astype(np.float64)
    with np.errstate(all='ignore'):
        c = pr[:, :2] + loc[:, :2] * float(F(0.1)) * pr[:, 2:]
        s = pr[:, 2:] * np.exp(loc[:, 2:] * float(F(0.2)))
        lo = c - s / 2
        return np.concatenate([lo, s + lo], 1)


def iou_matrix(bx, rcp=False):
    """[k,4] -> [k,k], entry (i, j) = IoU(box i, box j) in the dtype of bx, one operation per statement."""
    T = bx.dtype.type
    with np.errstate(all='ignore'):
        mx = np.minimum(bx[:, None, 2], bx[None, :, 2])
        mn = np.maximum(bx[:, None, 0], bx[None, :, 0])
        iw = mx - mn
        my = np.minimum(bx[:, None, 3], bx[None, :, 3])
        ny = np.maximum(bx[:, None, 1], bx[None, :, 1])
        ih = my - ny
        iw = np.where(iw < 0, T(0), iw)                 # (NaN stays NaN, as torch.clamp leaves it)
        ih = np.where(ih < 0, T(0), ih)
        inter = iw * ih
        w = bx[:, 2] - bx[:, 0]
        h = bx[:, 3] - bx[:, 1]
        area = w * h
        uni = area[:, None] + area[None, :]
        uni = uni - inter
        if rcp:
            r = T(1) / uni
            q = inter * r
        else:
            q = inter / uni
    assert q.dtype == bx.dtype
    return q


# ---- K2 ----------------------------------------------------------------------------------------------------------------------------

def ranked(score, kept_idx, k, ties_high=False):
    """The k best of kept_idx (ascending prior indices) by score descending, equal scores to the lowest (highest) index."""
    idx = kept_idx[::-1] if ties_high else kept_idx
    order = np.argsort(-score[idx].astype(np.float64), kind='stable')
    return idx[order[:k]]


def k2(k1o, loc, priors, top_k, nms_thresh, cross_class, variant=None, exp32=exp32_rounded, margins=True):
    """-> dict(cand_score [B,nclass,top_k], cand_prior, rank_prior (the selection before NMS, -1 padded), min_iou_margin (float64,
    over every pair i < j inside each (image, class)'s top-k), min_side / max_coord (float64, over the selected boxes),
    exact (float32 and float64 decode and IoU agree bit for bit after rounding))."""
    loc, priors = np.asarray(loc, F), np.asarray(priors, F)
    B, P = k1o['keep'].shape
    nclass = 1 if cross_class else k1o['scores_t'].shape[1]
    th = F(nms_thresh)
    cs = np.full((B, nclass, top_k), F(-1))
    cp = np.full((B, nclass, top_k), -1, np.int32)
    rp = np.full((B, nclass, top_k), -1, np.int32)
    margin, side, coord, exact = np.inf, np.inf, 0.0, True
    for b in range(B):
        kept = np.nonzero(k1o['keep'][b])[0]
        K = len(kept)
        if K == 0:
            continue
        k = min(K, top_k)
        tri = np.triu(np.ones((k, k), bool), 1)
        full = None
        if K <= 1024:          # boxes belong to priors, not to classes: one K x K matrix per image, indexed per class (same numbers)
            kb = decode32(loc[b, kept], priors[kept], exp32)
            full = [kb, iou_matrix(kb, rcp=(variant == 'rcp'))]
            if margins:
                k64 = decode64(loc[b, kept], priors[kept])
                full += [k64, iou_matrix(k64)]
            pos = np.full(P, -1)
            pos[kept] = np.arange(K)
        for c in range(nclass):
            sc = k1o['maxsc'][b] if cross_class else np.abs(k1o['scores_t'][b, c])
            sel = ranked(sc, kept, k, variant == 'ties_high')
            rp[b, c, :k] = sel
            if full is not None:
                q = pos[sel]
                bx, iou = full[0][q], full[1][np.ix_(q, q)]
            else:
                bx = decode32(loc[b, sel], priors[sel], exp32)
                iou = iou_matrix(bx, rcp=(variant == 'rcp'))
            if variant == 'nan_zero':
                iou = np.where(np.isnan(iou), F(0), iou)
            if margins:
                if full is not None:
                    b64, i64 = full[2][q], full[3][np.ix_(q, q)]
                else:
                    b64 = decode64(loc[b, sel], priors[sel])
                    i64 = iou_matrix(b64)
                with np.errstate(all='ignore'):
                    exact = exact and np.array_equal(b64.astype(F).view(np.int32), bx.view(np.int32)) \
                        and np.array_equal(i64.astype(F)[tri].view(np.int32), iou[tri].view(np.int32))
                    if k > 1:
                        m = np.abs(i64[tri] - float(th))
                        m = m[~np.isnan(m)]
                        if len(m):
                            margin = min(margin, float(m.min()))
                    fin = b64[np.isfinite(b64).all(1)]
                if len(fin):
                    side = min(side, float(min((fin[:, 2] - fin[:, 0]).min(), (fin[:, 3] - fin[:, 1]).min())))
                    coord = max(coord, float(np.abs(fin).max()))
            with np.errstate(all='ignore'):
                nan = (np.isnan(iou) & tri).any(0)
                mx = np.where(tri & ~np.isnan(iou), iou, F(0)).max(0)   # the maximum also runs over the zeroed lower triangle
                ok = ~nan & ((mx < th) if variant == 'lt' else (mx <= th))
            cs[b, c, :k][ok], cp[b, c, :k][ok] = sc[sel][ok], sel[ok]
    return dict(cand_score=cs, cand_prior=cp, rank_prior=rp, min_iou_margin=margin, min_side=side, max_coord=coord, exact=exact)


# ---- K3 ----------------------------------------------------------------------------------------------------------------------------

def k3(k1o, k2o, loc, coef, priors, top_k, max_det, cross_class, variant=None, exp32=exp32_rounded):
    """-> dict(count [B], box [B,cap,4], score, cls (int64), coef [B,cap,D], prior, rec [B, 1 + cap * (6 + D)]); rows >= count are 0."""
    loc, coef, priors = np.asarray(loc, F), np.asarray(coef, F), np.asarray(priors, F)
    B, nclass = k2o['cand_prior'].shape[:2]
    D = coef.shape[2]
    cap = top_k if cross_class else max_det
    o = dict(count=np.zeros(B, np.int32), box=np.zeros((B, cap, 4), F), score=np.zeros((B, cap), F),
             cls=np.zeros((B, cap), np.int64), coef=np.zeros((B, cap, D), F), prior=np.zeros((B, cap), np.int32),
             rec=np.zeros((B, 1 + cap * (6 + D)), F))
    for b in range(B):
        fs, fp = k2o['cand_score'][b].reshape(-1), k2o['cand_prior'][b].reshape(-1)
        valid = np.nonzero(fp >= 0)[0]
        n = min(len(valid), cap)
        o['count'][b] = n
        o['rec'][b, 0] = F(n)
        if n == 0:
            continue
        f = ranked(fs, valid, n, variant == 'ties_high')
        pri = fp[f]
        o['prior'][b, :n], o['score'][b, :n] = pri, fs[f]
        o['box'][b, :n] = decode32(loc[b, pri], priors[pri], exp32)
        o['cls'][b, :n] = k1o['argmax'][b, pri] if cross_class else f // top_k
        o['coef'][b, :n] = coef[b, pri]
        r = o['rec'][b, 1:].reshape(cap, 6 + D)
        r[:n, :4], r[:n, 4], r[:n, 5], r[:n, 6:] = o['box'][b, :n], o['score'][b, :n], o['cls'][b, :n].astype(F), o['coef'][b, :n]
    return o


def detect(case, variant=None, exp32=exp32_rounded, margins=True):
    """All three stages of a case (a dict as `make_case` builds it) -> dict(k1=, k2=, k3=)."""
    a = k1(case['conf'], case['C'], case['ld'], case['is_logits'], case['conf_thresh'], variant)
    b = k2(a, case['loc'], case['priors'], case['top_k'], case['nms_thresh'], case['cross_class'], variant, exp32, margins)
    c = k3(a, b, case['loc'], case['coef'], case['priors'], case['top_k'], case['max_det'], case['cross_class'], variant, exp32)
    return dict(k1=a, k2=b, k3=c)


def iou_bound(min_side, max_coord):
    """Bound on the change of an IoU when the device's expf is off by 2 ulp in w and h (see test_detect_kat_host.py
    test_random_cases_clear_their_margin for the derivation): 16 (e / m) (1 + e / m) + 2^-20 with e = 2^-21 M."""
    e = 2.0 ** -21 * max_coord
    r = e / min_side
    return 16 * r * (1 + r) + 2.0 ** -20


# ---- dispatch arithmetic of ymi_detect_f32 -----------------------------------------------------------------------------------------

def k2_branch(P, cross_class):
    """(EPT, SIGNED, load form) of class_topk_nms_k for buffers that start 16-byte aligned: row b > 0 (and class c > 0) starts at a
    multiple of P elements, so it is aligned exactly when P % 4 == 0, which is also the kernel's own first condition."""
    ept = 24 if P <= 24 * NT else 64 if P <= 64 * NT else 0
    return ('K2', ept, not cross_class, 'memory' if ept == 0 else 'vec' if P % 4 == 0 else 'scalar')


def k3_branch(C, top_k, cross_class):
    n = (1 if cross_class else C - 1) * top_k
    ept = 16 if n <= 16 * NT else 64 if n <= 64 * NT else 0
    return ('K3', ept, 'memory' if ept == 0 else 'vec' if n % 4 == 0 else 'scalar')


REACHABLE = set([('K2', e, s, f) for e in (24, 64) for s in (True, False) for f in ('vec', 'scalar')]
                + [('K2', 0, s, 'memory') for s in (True, False)] + [('K3', e, f) for e in (16, 64) for f in ('vec', 'scalar')])


def branches(case):
    return {k2_branch(case['P'], case['cross_class']), k3_branch(case['C'], case['top_k'], case['cross_class'])}


# ---- cases -------------------------------------------------------------------------------------------------------------------------

def make_case(name, family, conf, loc, priors, coef=None, C=None, ld=None, is_logits=False, top_k=200, max_det=100,
              conf_thresh=0.05, nms_thresh=0.5, cross_class=False, **extra):
    conf = np.ascontiguousarray(conf, F)
    B, P, ldc = conf.shape
    ld = ldc if ld is None else ld
    C = ld if C is None else C
    if coef is None:                                     # D = 4: prior index and image in the coefficients, exactly representable
        coef = np.zeros((B, P, 4), F)
        coef[:, :, 0] = np.arange(P)[None]
        coef[:, :, 1] = np.arange(B)[:, None]
        coef[:, :, 2] = -0.0
        coef[:, :, 3] = (np.arange(P)[None] % 7) * F(0.125)
    d = dict(name=name, family=family, conf=conf, loc=np.ascontiguousarray(loc, F), priors=np.ascontiguousarray(priors, F),
             coef=np.ascontiguousarray(coef, F), B=B, P=P, C=C, ld=ld, D=coef.shape[2], is_logits=bool(is_logits), top_k=top_k,
             max_det=max_det, conf_thresh=float(F(conf_thresh)), nms_thresh=float(F(nms_thresh)), cross_class=bool(cross_class))
    d.update(extra)
    return d


def scattered_boxes(rs, B, P, size=0.01):
    """Small boxes scattered over the unit square: priors [P,4] (cx, cy, w, h), loc [B,P,4]."""
    pri = np.empty((P, 4), F)
    pri[:, :2] = rs.rand(P, 2)
    pri[:, 2:] = rs.rand(P, 2) * size + size
    loc = (rs.randn(B, P, 4) * 0.1).astype(F)
    return pri, loc


def grid_boxes(P, cols=32):
    """Disjoint exact boxes: centres on a 2^-5 grid (odd multiples of 2^-6), sides 2^-6; with loc = 0 the decode is exact."""
    assert P <= cols * cols
    pri = np.empty((P, 4), F)
    i = np.arange(P)
    pri[:, 0] = (2 * (i % cols) + 1) / 64.0
    pri[:, 1] = (2 * (i // cols) + 1) / 64.0
    pri[:, 2:] = 1 / 64.0
    return pri


TIE = F(0.25)


def k2_tie_indices(P):
    s = {0, 3, 4, 4095, 4096, P - 2, P - 1}
    for g in range(1, P // 4096 + 1):
        s |= {4096 * g - 1, 4096 * g + 1}
    return sorted(i for i in s if 0 <= i < P)


def k2_dispatch_case(P, cross_class, seed):
    """Group 1.  B = 2, C = 3, top_k = 200.  Per image and class: 8 clear winners, then a tie at 0.25 of 3 x 192 = 576 priors or
    more (the listed indices and random ones) for the 192 slots left; 300 kept priors below the tie; everything else below
    conf_thresh.  Cross-class ranks the per-prior maximum: the union of the two classes' ties."""
    rs = np.random.RandomState(seed)
    B, C, top_k, nwin = 2, 3, 200, 8
    conf = np.full((B, P, C), 1e-4, F)
    conf[:, :, 0] = 0.9
    must = np.array(k2_tie_indices(P))
    ntie = 3 * (top_k - nwin) + 24
    for b in range(B):
        for c in (1, 2):
            if c == 1 or not cross_class:              # cross-class: one tie set for both classes, or the union would be twice as
                perm = rs.permutation(P)               # dense and the cut would fall below index 4095
            low = perm[:300]
            conf[b, low, c] = (0.06 + 0.15 * rs.rand(300)).astype(F)
            tied = np.union1d(must, perm[300:300 + ntie])
            conf[b, tied, c] = TIE
            win = perm[300 + ntie + nwin * (c - 1):300 + ntie + nwin * c]
            win = win[~np.isin(win, must)]
            conf[b, win, c] = (0.5 + 0.01 * np.arange(len(win))).astype(F) + F(0.1 * (c - 1))
    pri, loc = scattered_boxes(rs, B, P)
    return make_case('k2 P=%d %s' % (P, 'cc' if cross_class else 'pc'), 'tie', conf, loc, pri, top_k=top_k, max_det=100,
                     cross_class=cross_class, group=1, seed=seed, slots_left=top_k - nwin - (nwin if cross_class else 0))


K2_PS = (24574, 24576, 24577, 65536, 65537, 65539)
K3_SHAPES = [(81, 256, 256, 1), (66, 255, 100, 1), (4, 255, 1, 2), (65, 256, 100, 1)]   # C, top_k, max_det, B


def k3_dispatch_case(C, top_k, max_det, B, seed):
    """Group 2.  P = 320, K = 48 kept priors: every class holds 48 candidates (the other slots are -1), so the survivors (~48 per
    class) outnumber max_det except for C = 4 with max_det = 1.  Scores: 3 distinct winners in scattered classes (none for max_det = 1), then one value
    (0.25) shared by every kept prior in EVERY class: the final cut falls inside a tie that spans all classes, and class-major,
    rank-minor order decides."""
    rs = np.random.RandomState(seed)
    P, K = 320, 48
    conf = np.full((B, P, C), 1e-4, F)
    conf[:, :, 0] = 0.9
    for b in range(B):
        kept = np.sort(rs.permutation(P)[:K])
        conf[b, kept, 1:] = TIE
        # distinct scores above and below the tie in some classes, so the tie is neither first nor last
        for n, c in enumerate(rs.permutation(C - 1)[:3 if max_det > 3 else 0]):
            conf[b, kept[rs.randint(K)], 1 + c] = F(0.5 + 0.1 * n)
        for c in range(1, C, 2):
            lowp = kept[rs.permutation(K)[:5]]
            conf[b, lowp, c] = np.minimum(conf[b, lowp, c], (0.1 + 0.1 * rs.rand(5)).astype(F))
    pri, loc = scattered_boxes(rs, B, P)
    return make_case('k3 C=%d top_k=%d max_det=%d' % (C, top_k, max_det), 'tie', conf, loc, pri, top_k=top_k, max_det=max_det,
                     group=2, seed=seed)


TOPKS = (1, 2, 3, 9, 255, 256)


def selection_case(top_k, cross_class, seed):
    """Group 3.  P = 1024, C = 3; image b has K = 1, top_k - 1, top_k, top_k + 1 kept priors (those that are positive), random
    distinct scores."""
    rs = np.random.RandomState(seed)
    Ks = sorted({k for k in (1, top_k - 1, top_k, top_k + 1) if k > 0})
    B, P, C = len(Ks), 1024, 3
    conf = np.full((B, P, C), 1e-4, F)
    conf[:, :, 0] = 0.9
    for b, K in enumerate(Ks):
        kept = rs.permutation(P)[:K]
        conf[b, kept, 1] = (0.06 + 0.9 * rs.rand(K)).astype(F)
        conf[b, kept, 2] = (0.06 + 0.9 * rs.rand(K)).astype(F)
    pri, loc = scattered_boxes(rs, B, P)
    return make_case('select top_k=%d %s' % (top_k, 'cc' if cross_class else 'pc'), 'random', conf, loc, pri, top_k=top_k,
                     max_det=min(top_k, 100), cross_class=cross_class, group=3, seed=seed, Ks=Ks)


def triangle_pairs(k, seed=0, total=None):
    """Group 4: the (i, j), i < j, one per class.  k <= 17: all of them.  Else every row of the longest column, every (0, j), every
    (j - 1, j), and seeded random pairs up to `total`."""
    if k <= 17:
        return [(i, j) for j in range(k) for i in range(j)]
    s = {(i, k - 1) for i in range(k - 1)} | {(0, j) for j in range(1, k)} | {(j - 1, j) for j in range(1, k)}
    rs = np.random.RandomState(seed)
    while len(s) < total:
        j = rs.randint(1, k)
        s.add((rs.randint(0, j), j))
    return sorted(s)


def triangle_case(k, pairs, B):
    """Priors 0 and 1 carry the same box, every other prior a disjoint one (grid_boxes, loc = 0: exact).  Class c of image b puts
    prior 0 at rank i and prior 1 at rank j of its pair; the other ranks go to priors 2.. in order.  P = k + 8: K = P > top_k = k
    when all are kept, the last 8 never make the cut.  -> case with case['pairs'][b][c] = (i, j)."""
    P = k + 8
    ncls = -(-len(pairs) // B)
    C = ncls + 1
    assert C <= C_MAX
    conf = np.zeros((B, P, C), F)
    table = [[None] * ncls for _ in range(B)]
    rank_score = ((1000 - np.arange(P)) / 1024.0).astype(F)          # rank r -> score, distinct, all > conf_thresh
    for n in range(B * ncls):
        b, c = divmod(n, ncls)
        i, j = pairs[n % len(pairs)]
        table[b][c] = (i, j)
        others = iter(range(2, P))
        order = [0 if r == i else 1 if r == j else next(others) for r in range(P)]
        conf[b, order, 1 + c] = rank_score
    pri = grid_boxes(P)
    pri[1] = pri[0]
    return make_case('triangle k=%d' % k, 'exact', conf, np.zeros((B, P, 4), F), pri, top_k=k, max_det=min(k, 100), group=4,
                     pairs=table)


RCP_DIFFERS = [(5, 6), (3, 7), (6, 7), (9, 10), (9, 11), (5, 12), (7, 12), (3, 13), (6, 13), (12, 13), (3, 14), (9, 14), (11, 14),
               (13, 14)]         # fp32 a * (1 / b) != a / b
RCP_AGREES = [(1, 2), (1, 3), (3, 4), (2, 3), (1, 1)]


def threshold_case(a, b, which):
    """Group 5.  Box 0 = [1/4, 1/4, 1/4 + b/64, 1/2], box 1 = [1/4, 1/4, 1/4 + a/64, 1/2] (inside box 0): inter = a/256, union =
    b/256 exactly, IoU = fl(a / b) = q.  nms_thresh = prev(q) / q / next(q) for which = -1 / 0 / +1.  Two more disjoint priors."""
    q = F(a) / F(b)
    th = [prv(q), q, nxt(q)][which + 1]
    pri = np.array([[0.25 + b / 128.0, 0.375, b / 64.0, 0.25], [0.25 + a / 128.0, 0.375, a / 64.0, 0.25],
                    [0.75, 0.75, 1 / 64.0, 1 / 64.0], [0.875, 0.875, 1 / 64.0, 1 / 64.0]], F)
    conf = np.zeros((1, 4, 3), F)
    conf[0, :, 1] = [0.9, 0.8, 0.7, 0.6]
    conf[0, :, 2] = [0.8, 0.9, 0.6, 0.7]              # the other order: box 1 is the row, box 0 the column
    return make_case('iou %d/%d thresh %+d ulp' % (a, b, which), 'exact', conf, np.zeros((1, 4, 4), F), pri, top_k=4, max_det=8,
                     nms_thresh=th, group=5, ab=(a, b), which=which)


def degenerate_cases():
    """Group 6, each with its expected cand_prior of class 0 (prior indices by rank; -1 = suppressed)."""
    Z = np.zeros((1, 4, 4), F)
    conf = np.zeros((1, 4, 3), F)
    conf[0, :, 1] = [0.9, 0.8, 0.7, 0.6]
    conf[0, :, 2] = [0.6, 0.7, 0.8, 0.9]
    out = []
    pt = [0.5, 0.5, 0, 0]
    box = [0.5, 0.5, 0.25, 0.25]
    far = [0.125, 0.125, 1 / 64.0, 1 / 64.0]
    far2 = [0.875, 0.125, 1 / 64.0, 1 / 64.0]
    out.append(make_case('two zero-area boxes at one point', 'exact', conf, Z, np.array([pt, pt, far, far2], F), top_k=4,
                         max_det=8, group=6, want0=[0, -1, 2, 3]))
    out.append(make_case('zero-area box inside an ordinary one', 'exact', conf, Z, np.array([box, pt, far, far2], F), top_k=4,
                         max_det=8, group=6, want0=[0, 1, 2, 3]))
    inf = Z.copy()
    inf[0, 0, 2] = 1000.0
    out.append(make_case('infinite width as a row', 'exact', conf, inf, np.array([box, far, far2, pt], F), top_k=4, max_det=8,
                         group=6, want0=[0, -1, -1, -1]))
    inf = Z.copy()
    inf[0, 2, 2] = 1000.0
    out.append(make_case('infinite width as a column', 'exact', conf, inf, np.array([box, far, far2, pt], F), top_k=4, max_det=8,
                         group=6, want0=[0, 1, -1, -1]))
    touch = np.array([[0.25, 0.25, 0.25, 0.25], [0.5, 0.25, 0.25, 0.25], [0.3125, 0.3125, 0.125, 0.125], far2], F)
    out.append(make_case('nms_thresh 0: touching boxes stay, overlapping go', 'exact', conf, Z, touch, top_k=4, max_det=8,
                         nms_thresh=0.0, group=6, want0=[0, 1, -1, 3]))
    out.append(make_case('nms_thresh -0.5', 'exact', conf, Z, touch, top_k=4, max_det=8, nms_thresh=-0.5, group=6,
                         want0=[-1, -1, -1, -1]))
    half = np.array([[0.25, 0.25, 0.25, 0.25], [0.3125, 0.25, 0.125, 0.25], [0.75, 0.75, 0.125, 0.125], [0.75, 0.75, 0.125, 0.125]], F)
    out.append(make_case('IoU 0.5 at thresh 0.5, IoU 1 at thresh 0.5', 'exact', conf, Z, half, top_k=4, max_det=8, group=6,
                         want0=[0, 1, 2, -1]))
    out.append(make_case('IoU 1 at thresh 1.0', 'exact', conf, Z, half, top_k=4, max_det=8, nms_thresh=1.0, group=6,
                         want0=[0, 1, 2, 3]))
    return out


K1_SHAPES = [(2, 2), (3, 4), (4, 4), (81, 81), (81, 84), (81, 82), (234, 234), (234, 236)]
K1_PS = (1, 63, 64, 65, 700)
SCORE_BAR = 1e-6


def k1_case(C, ld, P, is_logits, seed):
    """Group 7.  B = 3, image 1 has K = 0.  Row p of images 0 and 2 is of kind (p + b) % 6.
    Post-softmax kinds: 0 ordinary kept, 1 maximum == conf_thresh (not kept), 2 maximum == next(conf_thresh) (kept), 3 below,
    4 / 5 foreground maxima tied across classes d = 1 + (p // 6) % 4 apart (kept / not kept).
    Logits kinds: 0, 3 ordinary (kept / background wins), 1 entries at +-80, 2 one entry 60 above the rest (its neighbours' scores
    are ~8.8e-27: exp(-60) does not underflow in float32; the +-80 rows are the ones whose low scores are exactly 0.0), 4, 5
    ordinary with a large margin.  The padding (ld > C) holds values that would win if they were read."""
    rs = np.random.RandomState(seed)
    B, th = 3, F(0.05)
    conf = np.empty((B, P, ld), F)
    for b in range(B):
        for p in range(P):
            kind = (p + b) % 6
            fg = C - 1
            if not is_logits:
                row = (0.001 + 0.03 * rs.rand(C)).astype(F)
                row[0] = 0.9
                c0 = 1 + rs.randint(fg)
                if b == 1:
                    row[c0] = prv(th) if p % 2 else th
                elif kind == 0:
                    row[c0] = F(0.2 + 0.5 * rs.rand())
                elif kind == 1:
                    row[c0] = th
                elif kind == 2:
                    row[c0] = nxt(th)
                elif kind >= 4:
                    d = 1 + (p // 6) % 4
                    c0 = 1 + rs.randint(max(1, fg - d))
                    v = F(0.3) if kind == 4 else F(0.04)
                    row[c0] = v
                    if c0 + d < C:
                        row[c0 + d] = v
                pad = 0.99
            else:
                row = rs.randn(C).astype(F)
                c0 = 1 + rs.randint(fg)
                if b == 1:
                    row[0] += 12
                elif kind == 0 or kind >= 4:
                    row[c0] += 8
                elif kind == 1:
                    row[:] = np.where(rs.rand(C) < 0.5, F(-80), F(-79))
                    row[c0] = 80
                elif kind == 2:
                    row[:] = -30
                    row[c0] = 30
                else:
                    row[0] += 12
                pad = 100.0
            conf[b, p, :C] = row
            conf[b, p, C:] = pad
    pri, loc = scattered_boxes(rs, B, P)
    return make_case('k1 C=%d ld=%d P=%d %s' % (C, ld, P, 'logits' if is_logits else 'scores'), 'k1', conf, loc, pri, C=C, ld=ld,
                     is_logits=is_logits, top_k=9, max_det=5, group=7, seed=seed, pass_ld=True)


def k1_sure(k1o, conf_thresh, bar=SCORE_BAR):
    """Rows of a fused-softmax case on which a device softmax within `bar` of the float64 one must give the reference's keep /
    argmax: the float64 maximum is further than `bar` from conf_thresh / than 2 x `bar` from the runner-up.  -> (keep_sure, argmax_sure) [B,P]."""
    fg = k1o['scores64'][:, :, 1:]
    top = fg.max(-1)
    if fg.shape[-1] > 1:
        second = np.sort(fg, -1)[:, :, -2]
    else:
        second = np.full_like(top, -np.inf)
    return np.abs(top - float(F(conf_thresh))) > bar, (top - second) > 2 * bar


def mixed_batch_case(seed):
    """Group 9.  B = 8, P = 24 577 (EPT 64, scalar loads), C = 3, top_k = 200.  K per image: 0, 1, 150, 200, 700 with a tie of 600 on
    the cut, 24 577 (all kept), 201, 0."""
    rs = np.random.RandomState(seed)
    B, P, C = 8, 24577, 3
    conf = np.full((B, P, C), 1e-4, F)
    conf[:, :, 0] = 0.9
    Ks = [0, 1, 150, 200, 700, P, 201, 0]
    for b, K in enumerate(Ks):
        kept = rs.permutation(P)[:K]
        for c in (1, 2):
            conf[b, kept, c] = (0.06 + 0.9 * rs.rand(K)).astype(F)
        if K == 700:
            conf[b, kept[:600], 1] = TIE
            conf[b, kept[600:], 1] = (0.3 + 0.6 * rs.rand(100)).astype(F)
            conf[b, kept, 2] = np.minimum(conf[b, kept, 2], TIE)
    pri, loc = scattered_boxes(rs, B, P)
    return make_case('mixed batch', 'random', conf, loc, pri, top_k=200, max_det=100, group=9, seed=seed, Ks=Ks)


def wrapper_case(cross_class, seed):
    """Group 10.  Detect(81, 0, 256, 0.05, 0.5), max_num_detections 256, P = 1024, B = 2, 300 / 40 kept priors."""
    rs = np.random.RandomState(seed)
    B, P, C = 2, 1024, 81
    conf = np.full((B, P, C), 1e-4, F)
    conf[:, :, 0] = 0.9
    for b, K in enumerate((300, 40)):
        kept = rs.permutation(P)[:K]
        for n, p in enumerate(kept):
            cls = rs.permutation(C - 1)[:3]
            conf[b, p, 1 + cls] = (0.06 + 0.9 * rs.rand(3)).astype(F)
    pri, loc = scattered_boxes(rs, B, P)
    coef = np.tanh(rs.randn(B, P, 32)).astype(F)
    return make_case('Detect top_k=256 %s' % ('cc' if cross_class else 'pc'), 'random', conf, loc, pri, coef=coef, top_k=256,
                     max_det=256, cross_class=cross_class, group=10, seed=seed)


def slice_image(case, b):
    d = dict(case)
    for k in ('conf', 'loc', 'coef'):
        d[k] = np.ascontiguousarray(case[k][b:b + 1])
    d['B'] = 1
    d['name'] = '%s [image %d]' % (case['name'], b)
    return d


# ---- the registry: every GPU case by id -------------------------------------------------------------------------------------------
# Seeds of the random-box cases: the first seed >= 1 at which the case's smallest deciding IoU margin (float64, from this reference
# alone) is at least 16 x iou_bound; test_detect_kat_host.py asserts that they hold.
SEEDS = {'k2-24574-pc': 8, 'k2-24576-pc': 2, 'k2-24577-cc': 3, 'k2-65536-pc': 2, 'k2-65537-pc': 3, 'k2-65537-cc': 2, 'sel-255-pc': 2,
         'sel-255-cc': 2, 'sel-256-pc': 6, 'sel-256-cc': 6, 'mixed': 5}


def case_ids(group):
    if group == 1:
        return ['k2-%d-%s' % (P, m) for P in K2_PS for m in ('pc', 'cc')]
    if group == 2:
        return ['k3-%d-%d-%d-%d' % s for s in K3_SHAPES]
    if group == 3:
        return ['sel-%d-%s' % (k, m) for k in TOPKS for m in ('pc', 'cc')]
    if group == 4:
        return ['tri-%d' % k for k in (2, 3, 4, 9, 17, 255, 256)]
    if group == 5:
        return ['iou-%d-%d-%s' % (a, b, 'm0p'[w + 1]) for a, b in RCP_DIFFERS + RCP_AGREES for w in (-1, 0, 1)]
    if group == 6:
        return ['deg-%d' % i for i in range(8)]
    if group == 7:
        return ['k1-%d-%d-%d-%s' % (C, ld, P, t) for C, ld in K1_SHAPES for P in K1_PS for t in ('scores', 'logits')]
    if group == 9:
        return ['mixed']
    if group == 10:
        return ['wrap-pc', 'wrap-cc']
    raise KeyError(group)


RANDOM_GROUPS = (1, 2, 3, 9, 10)


def build_case(cid, seed=None):
    f = cid.split('-')
    seed = SEEDS.get(cid, 1) if seed is None else seed
    if f[0] == 'k2':
        c = k2_dispatch_case(int(f[1]), f[2] == 'cc', seed)
    elif f[0] == 'k3':
        c = k3_dispatch_case(int(f[1]), int(f[2]), int(f[3]), int(f[4]), seed)
    elif f[0] == 'sel':
        c = selection_case(int(f[1]), f[2] == 'cc', seed)
    elif f[0] == 'tri':
        k = int(f[1])
        c = triangle_case(k, triangle_pairs(k, 0, 8 * (C_MAX - 1)), 1 if k <= 17 else 8)
    elif f[0] == 'iou':
        c = threshold_case(int(f[1]), int(f[2]), 'm0p'.index(f[3]) - 1)
    elif f[0] == 'deg':
        c = degenerate_cases()[int(f[1])]
    elif f[0] == 'k1':
        c = k1_case(int(f[1]), int(f[2]), int(f[3]), f[4] == 'logits', 1000 * int(f[1]) + int(f[3]))
    elif f[0] == 'mixed':
        c = mixed_batch_case(seed)
    elif f[0] == 'wrap':
        c = wrapper_case(f[1] == 'cc', seed)
    else:
        raise KeyError(cid)
    c['id'] = cid
    return c


def margin_ok(case, ref):
    """(smallest deciding margin, 16 x bound) of a random-box case."""
    k = ref['k2']
    return k['min_iou_margin'], 16 * iou_bound(k['min_side'], k['max_coord'])
