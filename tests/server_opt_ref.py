"""numpy restatement of the server-optimizer stage (include/fedavg/fa.h, "Server optimizer"): the expected
values of the server-optimizer tests.

Not a test module.  Every operation is one numpy fp32 operation followed by ``.astype(np.float32)``; nothing is
fused.  The aggregate ``avg`` is the fp32 value before any rounding to a 16-bit output: ``O.fedavg(...)`` for
FA_FEDAVG, ``trimmed_ref.trimmed_f32(...)`` for FA_TRIMMED.  bf16 values travel as ``np.uint16`` bit patterns.
"""
import numpy as np

from trimmed_ref import assert_bits, f32_to_bf16  # noqa: F401  (re-exported for the tests)

F32 = np.float32
NONE, MOMENTUM, ADAGRAD, ADAM, YOGI = 0, 1, 2, 3, 4
RULES = (MOMENTUM, ADAGRAD, ADAM, YOGI)
NAMES = {MOMENTUM: "momentum", ADAGRAD: "adagrad", ADAM: "adam", YOGI: "yogi"}


def f(a):
    return np.asarray(a).astype(F32)


def round_out(x, out="f32"):
    """x' in the out dtype: "f32", "f16" (np.float16) or "bf16" (np.uint16 bit patterns), rounded once."""
    x = np.ascontiguousarray(x, F32)
    if out == "f16":
        with np.errstate(over="ignore"):
            return x.astype(np.float16)
    if out == "bf16":
        return f32_to_bf16(x)
    return x.copy()


def step(rule, avg, x, m, v, lr, beta1=0.9, beta2=0.99, tau=1e-3):
    """One step: (x', m', v') in fp32; v' is None for MOMENTUM (v is not read)."""
    avg, x, m = (np.ascontiguousarray(a, F32) for a in (avg, x, m))
    lr, beta1, beta2, tau = F32(lr), F32(beta1), F32(beta2), F32(tau)
    c1, c2 = f(F32(1) - beta1), f(F32(1) - beta2)
    with np.errstate(all="ignore"):
        d = f(avg - x)
        if rule == MOMENTUM:
            m1 = f(f(beta1 * m) + d)
            return f(x + f(lr * m1)), m1, None
        v = np.ascontiguousarray(v, F32)
        m1 = f(f(beta1 * m) + f(c1 * d))
        q = f(d * d)
        if rule == ADAGRAD:
            v1 = f(v + q)
        elif rule == ADAM:
            v1 = f(f(beta2 * v) + f(c2 * q))
        elif rule == YOGI:
            u, s = f(c2 * q), f(v - q)
            v1 = np.full_like(v, np.nan)  # s is NaN
            v1 = np.where(s == 0, v, v1)
            v1 = np.where(s < 0, f(v + u), v1)
            v1 = f(np.where(s > 0, f(v - u), v1))
        else:
            raise ValueError("rule %r" % (rule,))
        x1 = f(x + f(f(lr * m1) / f(f(np.sqrt(v1)) + tau)))
        return x1, m1, v1


def bootstrap(rule, avg):
    """The first reduction of a part without a master: x' = avg, m' = v' = +0."""
    avg = np.ascontiguousarray(avg, F32)
    z = np.zeros_like(avg)
    return avg.copy(), z, (None if rule == MOMENTUM else z.copy())


def step64(rule, avg, x, m, v, lr, beta1=0.9, beta2=0.99, tau=1e-3):
    """The same formulas in float64 with the fp32 parameters (c1, c2 from the fp32 betas): the cross-check
    that catches a mistyped formula."""
    avg, x, m = (np.asarray(a, np.float64) for a in (avg, x, m))
    lr, beta1, beta2, tau = (np.float64(F32(p)) for p in (lr, beta1, beta2, tau))
    c1, c2 = np.float64(F32(1) - F32(beta1)), np.float64(F32(1) - F32(beta2))
    d = avg - x
    if rule == MOMENTUM:
        m1 = beta1 * m + d
        return x + lr * m1, m1, None
    v = np.asarray(v, np.float64)
    m1 = beta1 * m + c1 * d
    q = d * d
    if rule == ADAGRAD:
        v1 = v + q
    elif rule == ADAM:
        v1 = beta2 * v + c2 * q
    else:
        v1 = v - c2 * q * np.sign(v - q)
    return x + lr * m1 / (np.sqrt(v1) + tau), m1, v1
