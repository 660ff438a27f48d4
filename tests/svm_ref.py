"""float64 restatement of the linear-SVM problem behind fervit/directions.py (include/fervit.h fer_svm_forward,
fer_svm_xtr), shared by tests/test_svm_ref_cpu.py (against sklearn's LinearSVC) and the GPU tests.

Per class k: f_k(w, b) = 1/2 |w|^2 + 1/2 b^2 + sum_i c_i max(0, m_i)^2, m_i = 1 - s_i (w.x_i + b), s_i = +1 if
y_i == k else -1, c_i = Cp_k for positives, Cn_k for negatives: liblinear's L2-regularised squared hinge with a
regularised bias (intercept_scaling = 1). f_k is strongly convex with modulus 1, so for every theta = (w, b)
|theta - theta*| <= |grad f_k(theta)|: the optimality gate of tests/test_gpu_svm_fit.py needs no second solver.

A problem is the triple (s [N, K], c [N, K], reg_bias): `problem` builds the two methods' triples, the CPU test
builds slipped ones by hand; objective, gradient and the dense Newton solver take any triple."""
import numpy as np

# Gate of tests/test_gpu_svm_fit.py on |grad f_k| / |(w_k, b_k)| in float64 at the fp32 solution: 4 x the
# largest value measured on the MI355X over both methods and both shapes; never above
# GATE_CAP, beyond which the slips of tests/test_svm_ref_cpu.py would pass it.
GATE_CAP = 1e-3
GATE = 7.54e-4  # 4 x 1.884e-4 (binary, 600 x 96, class 3)


def weights(labels, K, method, C=0.1):
    """(Cp [K], Cn [K]) of sklearn's class_weight='balanced': binary = each class against the rest, balanced over
    the two sides; multiclass = the K-class fit, whose one-vs-rest problems weight only the positive side."""
    n = np.bincount(np.asarray(labels), minlength=K).astype(np.float64)
    N = float(n.sum())
    if method == "binary":
        return C * N / (2.0 * n), C * N / (2.0 * (N - n))
    assert method == "multiclass", method
    return C * N / (K * n), np.full(K, C)


def signs(labels, K):
    """s [N, K]: +1 where labels[i] == k, else -1."""
    return np.where(np.asarray(labels)[:, None] == np.arange(K)[None, :], 1.0, -1.0)


def problem(labels, K, method, C=0.1):
    """(s [N, K], c [N, K], reg_bias) of a method."""
    s = signs(labels, K)
    Cp, Cn = weights(labels, K, method, C)
    return s, np.where(s > 0, Cp[None, :], Cn[None, :]), True


def parts(X, W, b, s, c):
    """Z = X W^T + b, margins m = 1 - s Z, residual R = c a s m, curvature weights Dw = c a (a = [m > 0]) and the
    per-class loss sums of c a m^2; every array [N, K] but the loss [K]."""
    X, W, b = np.asarray(X, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    Z = X @ W.T + b[None, :]
    m = 1.0 - s * Z
    a = m > 0
    Dw = np.where(a, c, 0.0)
    return Z, m, Dw * s * m, Dw, (Dw * m * m).sum(0)


def objective(X, W, b, s, c, reg_bias=True):
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    return 0.5 * (W * W).sum(1) + (0.5 * b * b if reg_bias else 0.0) + parts(X, W, b, s, c)[4]


def gradient(X, W, b, s, c, reg_bias=True):
    """(grad_w [K, F], grad_b [K]) = (w - 2 X^T R, b - 2 sum R)."""
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    R = parts(X, W, b, s, c)[2]
    return W - 2.0 * R.T @ np.asarray(X, np.float64), (b if reg_bias else 0.0) - 2.0 * R.sum(0)


def relative_gradient(X, W, b, s, c, reg_bias=True):
    """|grad f_k| / |(w_k, b_k)| per class: by strong convexity an upper bound of the relative distance from the
    optimum."""
    gw, gb = gradient(X, W, b, s, c, reg_bias)
    W, b = np.asarray(W, np.float64), np.asarray(b, np.float64)
    return np.sqrt((gw * gw).sum(1) + gb * gb) / np.sqrt((W * W).sum(1) + b * b)


def newton(X, s, c, reg_bias=True, iters=200, gtol=1e-13):
    """The optimum by a dense Newton method with backtracking, class after class (small F): (W [K, F], b [K])."""
    X = np.asarray(X, np.float64)
    N, F = X.shape
    Xt = np.concatenate([X, np.ones((N, 1))], 1)
    reg = np.ones(F + 1)
    reg[F] = 1.0 if reg_bias else 0.0
    K = s.shape[1]
    out = np.zeros((K, F + 1))
    for k in range(K):
        sk, ck = s[:, k], c[:, k]

        def f_g(t):
            m = 1.0 - sk * (Xt @ t)
            a = m > 0
            return 0.5 * (reg * t * t).sum() + (ck * a * m * m).sum(), reg * t - 2.0 * Xt.T @ (ck * a * sk * m), a

        t = np.zeros(F + 1)
        f, g, a = f_g(t)
        g0 = np.linalg.norm(g)
        for _ in range(iters):
            if np.linalg.norm(g) <= gtol * g0:
                break
            H = np.diag(reg) + 2.0 * (Xt * (ck * a)[:, None]).T @ Xt
            d = np.linalg.solve(H + 1e-300 * np.eye(F + 1), -g)
            step = 1.0
            while True:
                fn, gn, an = f_g(t + step * d)
                if fn <= f + 1e-4 * step * (g @ d) or step < 1e-10:
                    break
                step *= 0.5
            t, f, g, a = t + step * d, fn, gn, an
        out[k] = t
    return out[:, :F], out[:, F]


def gaussian_classes(N, F, K=7, seed=0, spread=2.0):
    """(X fp32 [N, F], labels int64 [N]): K class means drawn N(0, spread^2 / F I) (norm about `spread`, so the
    classes overlap whatever F is), unit noise around them; class sizes unequal (class k gets a share
    proportional to k + 2), every class present."""
    g = np.random.default_rng(seed)
    share = np.arange(K) + 2.0
    labels = g.choice(K, size=N, p=share / share.sum())
    labels[:K] = np.arange(K)
    means = g.standard_normal((K, F)) * (spread / np.sqrt(F))
    X = means[labels] + g.standard_normal((N, F))
    return X.astype(np.float32), labels.astype(np.int64)
