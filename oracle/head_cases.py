"""Shape tables of the head / finalize / SGD / modality reference tests, and Python mirrors of
the launch arithmetic that decides which threads of a kernel do what (TEST INFRASTRUCTURE
ONLY).

``tests/test_gpu_head_ref.py`` runs the kernels over these tables; ``tests/test_oracle_head.py``
checks, without a GPU, that the tables reach every class a launch CAN reach, by enumerating
shapes through the mirrors below. Each mirror restates one piece of C++; when that changes,
its mirror (and, if a new class appears, the table) changes with it.

No form of these kernels is unreachable: every one has a single instantiation (the modality
kernel three, chosen by ``planes`` and the affine), and the classes below are all reached.
"""
from __future__ import annotations

import numpy as np

# --------------------------------------------------------------------------------------
# head.hip: head_moments_kernel / head_bwd_reduce_kernel
# --------------------------------------------------------------------------------------
K_HT = 256      # head.hip kHT: threads per workgroup
K_HU = 8        # head.hip kHU: rows in flight per thread


def head_form(V, M):
    """(Jc, G, tiles): columns per tile ``Jc = min(V*M, 256)``, row groups ``G = 256 // Jc``,
    column tiles ``ceil(J / Jc)``."""
    J = V * M
    Jc = min(J, K_HT)
    return Jc, K_HT // Jc, -(-J // Jc)


def j_class(V, M):
    """The class of a slab's column count J = V*M:
    "div"    J < 256 divides 256: G > 1 row groups, every thread owns a column;
    "idle"   J <= 128 does not divide 256: G > 1, threads with r >= G idle;
    "idle1"  128 < J < 256: G = 1 and idle threads;
    "full"   J = 256;  "ragged" J > 256, last tile partial;  "tiles" J > 256, exact tiles."""
    J = V * M
    Jc, G, tiles = head_form(V, M)
    if tiles > 1:
        return "tiles" if J % K_HT == 0 else "ragged"
    if J == K_HT:
        return "full"
    if K_HT % J == 0:
        return "div"
    return "idle" if G > 1 else "idle1"


def t_classes(T, G):
    """The classes of a frame count for G row groups (a thread takes rows r, r + G, ...,
    8 per trip): "T1"; "T<G" (row groups without a row); "T=8G" (one full trip exactly);
    "T=8G+1" (a second trip that holds one row, of group 0 alone); "T%G" (groups with
    different row counts)."""
    out = set()
    if T == 1:
        out.add("T1")
    if T < G:
        out.add("T<G")
    if T == G * K_HU:
        out.add("T=8G")
    if T == G * K_HU + 1:
        out.add("T=8G+1")
    if G > 1 and T % G:
        out.add("T%G")
    return out


def reachable_head_classes(max_J=1100):
    """Every (j_class, t_class) pair some clip reaches (M = 1: the classes depend on V*M)."""
    out = set()
    for J in range(1, max_J):
        G = head_form(J, 1)[1]
        for T in list(range(1, 12)) + [G - 1, G * K_HU, G * K_HU + 1, G * K_HU + 2]:
            if T >= 1:
                out |= {(j_class(J, 1), tc) for tc in t_classes(T, G)}
    return out


def _head_clips():
    # (V, M) of the column counts J = 1, 2, 32, 64 (dividing 256), 50, 33, 75 (idle threads,
    # G > 1), 150 (idle threads, G = 1), 256, 300 (ragged), 512 (two exact tiles)
    vm = [(1, 1), (1, 2), (2, 1), (16, 2), (32, 2), (25, 2), (11, 3), (33, 1), (25, 3),
          (50, 3), (128, 2), (256, 1), (100, 3), (256, 2)]
    clips = []
    k = 0
    for V, M in vm:
        G = head_form(V, M)[1]
        Ts = {1, G * K_HU, G * K_HU + 1}
        if G > 2:
            Ts |= {G - 1}
        if G > 1:
            Ts |= {G + 1, 3 * G - 1}          # not a multiple of G, below and inside one trip
        else:
            Ts |= {2, 20}                     # G = 1: a short first trip, a short third trip
        for T in sorted(Ts):
            N, C = (1, 3)[k % 2], (1, 2, 3)[k % 3]
            clips.append((N, C, T, V, M))
            k += 1
    return clips


#: (N, C, T, V, M) clips of the four head kernels.
HEAD_CLIPS = _head_clips()
#: The conditioning columns of sgcn_head_moments run at these clips, every column alike.
COND_CLIPS = [(2, 3, 300, 25, 2), (2, 3, 64, 25, 2), (1, 3, 300, 33, 1), (1, 2, 64, 100, 3)]
#: Column (c) also where a thread adds 300 rows alone and the bound on q/M2 is lowest.
COND_EDGE_CLIPS = COND_CLIPS + [(1, 1, 300, 100, 3)]


def cond_clip(shape, kind):
    """A clip whose every column is an adversarial one: ``kind`` "a": a joint missing (0) in
    the first frame and nearly still afterwards (2 + 0.05 * noise); "b": an outlier (5) in the
    first frame, then constant (1.37); "c": noise about 1 whose first frame sits where the
    kernel decides whether to sum a column again (q/M2 = head_cond), times 0.8 .. 1.2 across
    the columns, so that both decisions occur and the first-frame sums are kept at the worst
    conditioning they are ever kept at."""
    import formula
    import torch
    N, C, T, V, M = shape
    if kind == "a":
        x = 2.0 + 0.05 * formula.tensor(shape, 4242, 1.0)
        x[:, :, 0] = 0.0
    elif kind == "b":
        x = torch.full(shape, 1.37)
        x[:, :, 0] = 5.0
    elif kind == "c":
        x = 1.0 + formula.tensor(shape, 4243, 1.0)
        rest = x[:, :, 1:].double()
        # the other T - 1 frames have mean mu and deviation s: x0 = mu + z*s gives the whole
        # column q/M2 = 1 + z*z*(T - 1)/(T + z*z)
        k = float(head_cond(T, head_form(V, M)[1]))
        z = float(np.sqrt((k - 1.0) * T / (T - k)))
        w = torch.linspace(0.8, 1.2, V * M, dtype=torch.float64).reshape(V, M)
        x[:, :, 0] = (rest.mean(2) + rest.std(2, unbiased=False) * z * w).float()
    else:
        raise ValueError(kind)
    return x.float()


def head_inputs(clip):
    """The operands of the four head kernels at one clip: the clip and the plane gradient
    offset from zero (no column sum near zero: tests/test_oracle_head.py), statistics and
    coefficients in data_bn's feature order."""
    import formula
    t = formula.tensor
    N, C, T, V, M = clip
    F = M * V * C
    return dict(x=t(clip, 1001, 2.0, 1.0), g=t((N * M, C, T, V), 1002, 1.0, 0.5),
                mean=t((F,), 1003, 0.3), invstd=t((F,), 1004, 0.4, 1.0),
                scale=t((F,), 1005, 0.5, 1.0), shift=t((F,), 1006, 0.2),
                coef=t((3, F), 1007, 0.5, 0.25))


K_HCOND = 20.0          # head.hip kHCond
K_HCOND_ROWS = 1200.0   # head.hip kHCondRows


def head_cond(T, G):
    """head_moments_kernel's bound on q/M2 of the first-frame sums, in float32: above it a
    column is summed again about its mean."""
    f = np.float32
    return min(f(K_HCOND), f(K_HCOND_ROWS) / f((T + G - 1) // G))


def emulate_head_moments(x, pivot="kernel", with_again=False):
    """head_moments_kernel's float32 arithmetic in numpy (sums in the kernel's order: a row
    group's rows ascending, then the groups ascending; products and sums each rounded, no
    fused multiply-add). (N, F, 2) like the kernel's output.

    ``pivot="first"``: the shifted sums pivot on the column's FIRST FRAME alone, as the kernel
    did before this suite: ``k0 = x[0]; a = sum (x - k0); q = sum (x - k0)^2; mean = k0 + a/T;
    M2 = q - a*a/T``. Kept to show what that pivot costs.
    ``pivot="mean"``: every column summed a second time about that mean ``mu``:
    ``a2 = sum (x - mu); q = sum (x - mu)^2; mean = mu + a2/T; M2 = q - a2*a2/T``.
    ``pivot="kernel"``: the kernel: the first-frame result where ``q <= head_cond * M2``, the
    second sum elsewhere. ``with_again``: also return which columns were summed again, in
    the output's feature order."""
    f = np.float32
    xs = np.asarray(x, dtype=f)
    N, C, T, V, M = xs.shape
    G = head_form(V, M)[1]
    nT = f(T)

    def sums(k):
        ta, tq = np.zeros_like(k), np.zeros_like(k)
        for g in range(G):
            a, q = np.zeros_like(k), np.zeros_like(k)
            for t in range(g, T, G):
                d = (xs[:, :, t] - k).astype(f)
                a = (a + d).astype(f)
                q = (q + (d * d).astype(f)).astype(f)
            ta, tq = (ta + a).astype(f), (tq + q).astype(f)
        return ta, tq

    def result(k, ta, tq):
        return ((k + (ta / nT).astype(f)).astype(f),
                (tq - ((ta * ta).astype(f) / nT).astype(f)).astype(f))

    k = xs[:, :, 0]                                        # (N, C, V, M)
    ta, tq = sums(k)
    mean, m2 = result(k, ta, tq)
    if pivot == "first":
        again = np.zeros(k.shape, bool)
    elif pivot == "mean":
        again = np.ones(k.shape, bool)
    elif pivot == "kernel":
        with np.errstate(invalid="ignore"):
            again = tq > (head_cond(T, G) * m2).astype(f)
    else:
        raise ValueError(pivot)
    if again.any():
        mean2, m22 = result(mean, *sums(mean))
        mean, m2 = np.where(again, mean2, mean), np.where(again, m22, m2)

    def order(v):
        return v.transpose(0, 3, 2, 1).reshape(N, M * V * C)   # (N, C, V, M) -> (N, F)
    out = np.stack((order(mean), order(m2)), -1)
    return (out, order(again)) if with_again else out


# --------------------------------------------------------------------------------------
# head.hip: pool_kernel (4 x 256 elements per trip) and pool_bwd_kernel (float4 stores)
# --------------------------------------------------------------------------------------
POOL_P = [1, 5, 255, 256, 1023, 1024, 1025, 2049]
POOL_M = [1, 2, 3]
#: (N, M, C, P) of sgcn_pool / sgcn_pool_bwd / sgcn_pool_bwd_planes.
POOL_CASES = [(2, M, 3, P) for P in POOL_P for M in POOL_M] + [
    (1, 1, 3, 5),       # a total that is no multiple of 4: the scalar tail stores
    (2, 2, 3, 7),       # a multiple of 4 whose rows begin mid-vector
    (3, 1, 1, 1), (1, 3, 5, 1)]


def pool_class(P):
    """How pool_kernel's trips of 4 x 256 elements meet a plane of P elements."""
    full, rest = divmod(P, 4 * K_HT)
    return (min(full, 2), "none" if rest == 0 else "lt256" if rest < K_HT else
            "eq256" if rest == K_HT else "gt256")


def pool_bwd_class(N, M, C, P):
    """pool_bwd_kernel: ("tail" | "whole" last vector, vectors that span two rows or not)."""
    total = N * M * C * P
    return ("tail" if total % 4 else "whole", "straddle" if P % 4 else "rows")


# --------------------------------------------------------------------------------------
# bn.hip: feature_sums (8 waves over the batch, 4 rows in flight, 64 features per workgroup)
# --------------------------------------------------------------------------------------
K_FSW = 8
FIN_B = [1, 2, 7, 8, 9, 24, 25, 32, 33, 40, 64, 65,
         41, 49]        # two and three remainder rows after an unrolled trip
FIN_F = [1, 63, 64, 65, 150, 1600, 66]          # 66 = 2 x 33: a per-joint case above one wave


def fin_perm_Vs(F):
    return [0] + ([25] if F == 1600 else []) + ([33] if F % 33 == 0 else [])


def fin_wave_rows(B, w):
    """(unrolled trips, remainder rows) of wave ``w``: ``for (b = w; b + 24 < B; b += 32)``
    then ``for (; b < B; b += 8)``."""
    b, trips, rem = w, 0, 0
    while b + 3 * K_FSW < B:
        trips, b = trips + 1, b + 4 * K_FSW
    while b < B:
        rem, b = rem + 1, b + K_FSW
    return trips, rem


def fin_classes(B):
    """The (trips capped at 2, remainder rows) of the 8 waves."""
    return {(min(t, 2), r) for t, r in (fin_wave_rows(B, w) for w in range(K_FSW))}


def fin_f_class(F):
    """(one workgroup or more, lanes of the last workgroup past F clamped or not)."""
    return (min(-(-F // 64), 2), F % 64 != 0)


# --------------------------------------------------------------------------------------
# optim.hip: sgd_step_kernel (2048-element chunks, 256 threads)
# --------------------------------------------------------------------------------------
SGD_CHUNK = 2048
SGD_THREADS = 256
SGD_NUMEL = [1, 255, 256, 257, 2047, 2048, 2049, 4097, 5000]


def sgd_layout(numels=SGD_NUMEL):
    """(offsets, arena size): the tensors carved from one arena at odd element offsets, 1 to 3
    elements of sentinel either side of each."""
    offs, o = [], 1
    for k, n in enumerate(numels):
        offs.append(o)
        gap = 1 + k % 3
        if (o + n + gap) % 2 == 0:             # the next offset is odd
            gap += 1 if gap < 3 else -1
        o += n + gap
    return offs, o + 2


def sgd_chunks(numels=SGD_NUMEL, seed=5):
    """The {tensor, first element} chunk map in a shuffled (fixed) order."""
    ch = [(t, s) for t, n in enumerate(numels) for s in range(0, n, SGD_CHUNK)]
    return [ch[i] for i in np.random.RandomState(seed).permutation(len(ch))]


def f32_bits(v):
    return int(np.float32(v).view(np.uint32))


def sgd_table(ptrs, wd_lr, flags, scales):
    """The (n, 5) int64 table of sgcn_sgd_step: ``ptrs`` [(param, grad, buf) addresses];
    ``wd_lr`` [(wd, lr) floats, or a device address when flags bit 2 is set]."""
    rows = []
    for (p, g, b), h, fl, s in zip(ptrs, wd_lr, flags, scales):
        col = h if fl & 4 else f32_bits(h[0]) | f32_bits(h[1]) << 32
        rows.append([p, g, b, col, fl | (f32_bits(s) << 32 if fl & 2 else 0)])
    return np.array(rows, dtype=np.uint64).view(np.int64)


# --------------------------------------------------------------------------------------
# ensemble.hip: modalities_kernel
# --------------------------------------------------------------------------------------
MOD_VM = [(7, 3), (25, 2), (33, 1)]
MOD_C = [1, 3, 4]
MOD_T = [1, 2, 9]
MOD_N = 2


def synthetic_parent(V):
    """A parent table no skeleton has: several self-parents (the first, a middle and the last
    joint) and parents above their child."""
    par = np.array([V - 1 - v for v in range(V)], dtype=np.int32)
    for v in (0, V // 2, V - 1):
        par[v] = v
    return par
