"""The fused SAC update without a GPU: the arithmetic and the summation order of gym-usv_amd/csrc/usv_sac_math.hpp
through a stand-alone host program built with AddressSanitizer and UBSan, compared bit for bit with the NumPy
restatement (tests/sac_loss_ref.py); the restatement against torch-CPU float64 autograd of SB3's lines under the
1e-5 ceiling; the argument refusals of the new C entries; and the Python ValueErrors that need no device."""
import ctypes
import subprocess

import numpy as np
import pytest

import sac_loss_ref as S

MAIN = r"""
#include <cstdio>
#include <vector>
#include "usv_sac_math.hpp"
using namespace usv;

// stdin, repeated until the end of the input: a header of 3 int64 (kind, n, flags), then
//   kind 0, critic (flags: 1 entropy term, 2 per-row discounts): q1 q2 q1t q2t rew done [logp_next] [disc] [n] f32 each,
//           ent gamma f32.           stdout: target g_q1 g_q2 [n], loss
//   kind 1, policy (flags: 1 log_ent): logp q1 q2 [n], ent log_ent te f32.
//                                    stdout: g_logp g_q1 g_q2 [n], actor_loss ent_coef_loss g_log_ent (0 without log_ent)
//   kind 2, Polyak: tau f64, t p [n]. stdout: t' [n]
//   kind 3, scale (flags: 1 an upstream is given): g [n], up f32.   stdout: o [n]
static bool rd(std::vector<float>& v) { return std::fread(v.data(), 4, v.size(), stdin) == v.size(); }
static void wr(const std::vector<float>& v) { std::fwrite(v.data(), 4, v.size(), stdout); }

int main() {
  int64_t h[3];
  while (std::fread(h, 8, 3, stdin) == 3) {
    const int64_t n = h[1], fl = h[2];
    if (n < 1) return 4;
    std::vector<float> a(n), b(n), c(n), d(n), e(n), f(n), g(n), k(n), o1(n), o2(n), o3(n), t1(n), t2(n), t3(n);
    if (h[0] == 0) {
      float sc[2];
      if (!rd(a) || !rd(b) || !rd(c) || !rd(d) || !rd(e) || !rd(f) || ((fl & 1) && !rd(g)) || ((fl & 2) && !rd(k)) ||
          std::fread(sc, 4, 2, stdin) != 2) return 3;
      for (int64_t i = 0; i < n; ++i) {
        o1[i] = sac_target(c[i], d[i], (fl & 1) != 0, sc[0], (fl & 1) ? g[i] : 0.0f, e[i], f[i], (fl & 2) ? k[i] : sc[1]);
        sac_critic_row(a[i], b[i], o1[i], n, t1[i], t2[i], o2[i], o3[i]);
      }
      const float loss = sac_critic_loss(sac_sum(t1.data(), n), sac_sum(t2.data(), n), n);
      wr(o1), wr(o2), wr(o3);
      std::fwrite(&loss, 4, 1, stdout);
    } else if (h[0] == 1) {
      float sc[3];
      if (!rd(a) || !rd(b) || !rd(c) || std::fread(sc, 4, 3, stdin) != 3) return 3;
      for (int64_t i = 0; i < n; ++i) {
        sac_policy_row(a[i], b[i], c[i], sc[0], (fl & 1) ? sc[1] : 0.0f, sc[2], n, t1[i], t2[i], t3[i], o2[i], o3[i]);
        o1[i] = sac_mean(sc[0], n);
      }
      float out[3] = {sac_mean(sac_sum(t1.data(), n), n), 0.0f, 0.0f};
      if (fl & 1) out[1] = sac_neg_mean(sac_sum(t2.data(), n), n), out[2] = sac_neg_mean(sac_sum(t3.data(), n), n);
      wr(o1), wr(o2), wr(o3);
      std::fwrite(out, 4, 3, stdout);
    } else if (h[0] == 2) {
      double tau;
      if (std::fread(&tau, 8, 1, stdin) != 1 || !polyak_tau_ok(tau) || !rd(a) || !rd(b)) return 3;
      float tau_f, om;
      polyak_coeffs(tau, tau_f, om);
      if (polyak_chunks(n) != (n + kPolyakChunk - 1) / kPolyakChunk) return 5;
      for (int64_t i = 0; i < n; ++i) o1[i] = polyak_value(a[i], b[i], tau_f, om);
      wr(o1);
    } else if (h[0] == 3) {
      float up;
      if (!rd(a) || std::fread(&up, 4, 1, stdin) != 1) return 3;
      for (int64_t i = 0; i < n; ++i) o1[i] = (fl & 1) ? a[i] * up : 0.0f;
      wr(o1);
    } else {
      return 6;
    }
  }
  std::fprintf(stderr, "P %d C %d scratch %zu %zu\n", kSacPartialRows, kPolyakChunk, sac_scratch_floats(1),
               sac_scratch_floats(2 * kSacPartialRows + 1));
  return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """The program with AddressSanitizer + UBSan: a stand-alone host binary, run directly."""
    from gym_usv_amd.build import CSRC, hipcc
    d = tmp_path_factory.mktemp("sac_loss_math")
    src, exe = d / "sac.cpp", d / "sac_san"
    src.write_text(MAIN)
    subprocess.run([hipcc(), "-x", "c++", "-std=c++17", "-Wall", "-O1", "-g", f"-I{CSRC}",
                    "-fsanitize=address,undefined", "-fno-gpu-sanitize", "-fno-sanitize-recover=all",
                    "-o", str(exe), str(src)], check=True)
    return str(exe)


def run(exe, records):
    """`records`: [(kind, n, flags, [arrays and scalars in the program's order], output floats)]; one run."""
    parts = []
    for kind, n, flags, items, _ in records:
        parts.append(np.array([kind, n, flags], np.int64))
        parts += [np.ascontiguousarray(x) for x in items]
    p = subprocess.run([exe], input=b"".join(x.tobytes() for x in parts), capture_output=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr.decode(errors="replace")[-2000:])
    assert p.stderr.decode().strip() == f"P {S.P} C {S.C} scratch 7 13"
    out, at = [], 0
    for *_, count in records:
        out.append(np.frombuffer(p.stdout, np.float32, count, at))
        at += 4 * count
    assert at == len(p.stdout)
    return out


def critic_record(x, form):
    flags = {"disc": 3, "gamma": 1, "td3": 0}[form]
    items = [x[k] for k in ("q1", "q2", "q1t", "q2t", "rew", "done")]
    items += [x["logp_next"]] * (flags & 1) + [x["disc"]] * (flags >> 1)
    return (0, len(x["q1"]), flags, items + [np.array([x["ent"], x["gamma"]], np.float32)], 3 * len(x["q1"]) + 1)


def policy_record(x, with_le=True):
    B = len(x["logp"])
    return (1, B, int(with_le), [x["logp"], x["q1p"], x["q2p"], np.array([x["ent"], x["log_ent"], x["te"]], np.float32)],
            3 * B + 3)


def policy_ref(x, with_le=True):
    return S.policy(x["logp"], x["q1p"], x["q2p"], x["ent"], *((x["log_ent"], x["te"]) if with_le else ()))


def test_losses_equal_the_restatement_bitwise(program):
    cases, records = [], []
    for B in S.ROWS:
        for j, form in enumerate(S.CRITIC_FORMS):
            x = S.inputs(B, seed=j, ent=0.0 if (form == "gamma" and B % 2) else 0.2)
            cases.append(("critic", B, form, x))
            records.append(critic_record(x, form))
        for with_le in (True, False):
            x = S.inputs(B, seed=3 + with_le)
            cases.append(("policy", B, with_le, x))
            records.append(policy_record(x, with_le))
    for (kind, B, form, x), got in zip(cases, run(program, records)):
        if kind == "critic":
            a, kw = S.critic_case(x, form)
            want = S.critic(*a, **kw)
            names = ("target", "g_q1", "g_q2")
            assert set(np.unique(x["done"])) <= {0.0, 1.0} and (B < 2 or len(np.unique(x["done"])) == 2)
        else:
            want = policy_ref(x, form)
            names = ("g_logp", "g_q1", "g_q2")
            if B >= 5:
                assert (x["q1p"] == x["q2p"]).any() and (x["q1p"] < x["q2p"]).any() and (x["q1p"] > x["q2p"]).any()
        for i, name in enumerate(names):
            assert S.same(got[i * B:(i + 1) * B], want[name]), (kind, B, form, name)
        tail = got[3 * B:]
        if kind == "critic":
            assert S.same(tail, [want["loss"]]), (B, form, tail, want["loss"])
        elif form:
            assert S.same(tail, [want["actor_loss"], want["ent_coef_loss"], want["g_log_ent"]]), (B, tail, want)
        else:
            assert S.same(tail, [want["actor_loss"], 0.0, 0.0]), (B, tail, want)


def test_a_nan_in_q2_pi_alone_reaches_the_actor_loss(program):
    for B in (5, S.P + 1):
        x = S.inputs(B, nan_q2_pi=True)
        assert np.isnan(x["q2p"]).sum() == 1 and not np.isnan(x["q1p"]).any()
        got, = run(program, [policy_record(x)])
        want = policy_ref(x)
        assert np.isnan(want["actor_loss"]) and np.isnan(got[3 * B])
        assert not np.isnan(got[3 * B + 1]) and S.same(got[3 * B + 1:], [want["ent_coef_loss"], want["g_log_ent"]])
    # the other operand, and the critic's min
    assert np.isnan(S.policy(x["logp"], x["q2p"], x["q1p"], x["ent"])["actor_loss"])
    y = dict(x, q1t=x["q2p"])
    got, = run(program, [critic_record(y, "disc")])
    assert np.isnan(got[B // 2]) and np.isnan(got[3 * B]) and np.isnan(got[:B]).sum() == 1


def test_the_sum_is_the_fixed_order_and_not_a_sequential_one(program):
    """Cases whose sequential float32 sum gives another loss than the partial-strand-tree one (four seeds, so that
    the two do not agree by chance in all): the program gives the latter in every one."""
    B, differ = 2 * S.P + 1, 0
    xs = [S.inputs(B, seed=11 + j) for j in range(4)]
    for x, got in zip(xs, run(program, [critic_record(x, "disc") for x in xs])):
        a, kw = S.critic_case(x, "disc")
        want = S.critic(*a, **kw)
        d1, d2 = x["q1"] - want["target"], x["q2"] - want["target"]
        seq = [np.float32(0.0), np.float32(0.0)]
        for i in range(B):
            seq[0], seq[1] = seq[0] + d1[i] * d1[i], seq[1] + d2[i] * d2[i]
        seq_loss = np.float32(0.5) * (seq[0] / np.float32(B) + seq[1] / np.float32(B))
        assert S.same(got[3 * B:], [want["loss"]])
        differ += not S.same([seq_loss], [want["loss"]])
    assert differ > 0


def test_polyak_and_scale_equal_the_restatement_bitwise(program):
    records, want = [], []
    for n in S.NUMELS:
        for tau in S.TAUS:
            rng = np.random.default_rng(n)
            t, p = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
            records.append((2, n, 0, [np.array([tau], np.float64), t, p], n))
            want.append(S.polyak(t, p, tau))
    g = S.inputs(257)["q1"]
    for up in (1.0, -0.37, None):
        records.append((3, 257, int(up is not None), [g, np.array([up or 0.0], np.float32)], 257))
        want.append(S.scaled(g, up))
    for got, w in zip(run(program, records), want):
        assert S.same(got, w)
    t, p = np.float32([1.5, -2.0]), np.float32([0.25, 7.0])
    assert S.same(S.polyak(t, p, 0.0), t) and S.same(S.polyak(t, p, 1.0), p)
    assert S.polyak_coeffs(0.005) == (np.float32(0.005), np.float32(0.995))


def test_the_restatement_is_within_the_ceiling_of_the_definition():
    """The float32 order against torch-CPU float64 autograd of SB3's lines, errors over the sums of magnitudes."""
    worst = {}
    for B in S.ROWS:
        for j, form in enumerate(S.CRITIC_FORMS):
            x = S.inputs(B, seed=j)
            a, kw = S.critic_case(x, form)
            for k, v in S.errors(S.critic(*a, **kw), S.torch_critic(*a, **kw), S.critic_scales(*a, **kw)).items():
                worst["critic " + k] = max(worst.get("critic " + k, 0.0), v)
        x = S.inputs(B, seed=4)
        a = (x["logp"], x["q1p"], x["q2p"], x["ent"], x["log_ent"], x["te"])
        for k, v in S.errors(S.policy(*a), S.torch_policy(*a), S.policy_scales(*a)).items():
            worst["policy " + k] = max(worst.get("policy " + k, 0.0), v)
    print(worst)
    assert len(worst) == 10 and all(v < S.CEILING for v in worst.values()), worst


@pytest.fixture(scope="module")
def lib():
    from gym_usv_amd import _lib
    from gym_usv_amd.build import build_library
    build_library(verbose=False)
    return _lib.load()


def test_entries_refuse_bad_arguments_without_gpu(lib):
    """Everything the new entries can refuse before a HIP call is refused with USV_ERR_ARG and a message."""
    from gym_usv_amd import _lib
    assert _lib.ABI_VERSION == 5 == lib.usv_abi_version()
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16

    def refused(rc, word):
        assert rc == -1 and word in lib.usv_last_error(), (word, rc, lib.usv_last_error())

    assert [lib.usv_sac_scratch_floats(r) for r in (-1, 0, 1, S.P, S.P + 1)] == [0, 0, 7, 7, 10]

    def critic(word, rows=5, ent=p, logp_next=p, req=(p,) * 8, g=(p, p), scratch=p):
        q1, q2, q1n, q2n, rew, done, target, loss = req
        refused(lib.usv_sac_critic_loss(rows, q1, q2, q1n, q2n, rew, done, ent, logp_next, None, 0.99, target, loss, *g,
                                        scratch, None), word)

    for rows in (0, -4):
        critic(b"rows must be >= 1", rows=rows)
    critic(b"both NULL or both set", ent=None)
    critic(b"both NULL or both set", logp_next=None)
    critic(b"null buffer", scratch=None)
    critic(b"not 16-B aligned", scratch=p + 4)
    for i in range(8):
        critic(b"null buffer", req=tuple(None if j == i else p for j in range(8)))
        critic(b"not 4-B aligned", req=tuple(p + 2 if j == i else p for j in range(8)))
    critic(b"not 4-B aligned", g=(p + 1, None))

    def policy(word, rows=5, req=(p,) * 4, log_ent=p, actor=p, ent_loss=p, g=(None,) * 4, scratch=p):
        refused(lib.usv_sac_policy_loss(rows, *req, log_ent, -2.0, actor, ent_loss, *g, scratch, None), word)

    policy(b"rows must be >= 1", rows=0)
    policy(b"log_ent needs ent_loss", ent_loss=None)
    policy(b"null buffer", actor=None)
    policy(b"null buffer", scratch=None)
    for i in range(4):
        policy(b"null buffer", req=tuple(None if j == i else p for j in range(4)))
        policy(b"not 4-B aligned", g=tuple(p + 2 if j == i else None for j in range(4)))

    def backward(word, rows=5, up=p, g=(p, p, p), o=(p, p, p), up_s=p, gs=p, os=p):
        refused(lib.usv_sac_loss_backward(rows, up, *g, *o, up_s, gs, os, None), word)

    backward(b"rows must be >= 1", rows=0)
    backward(b"null buffer", o=(None, p, p))
    backward(b"null buffer", g=(None, p, p))
    backward(b"without its unit gradient", g=(p, None, p))
    backward(b"without its unit gradient", gs=None)
    backward(b"not 4-B aligned", up=p + 2)

    Pair = _lib.UsvPolyakPair

    def polyak(word, pairs, n=None, table=p, nbytes=1 << 20, tau=0.005):
        arr = (Pair * len(pairs))(*pairs) if pairs is not None else None
        refused(lib.usv_polyak_update(arr, len(pairs) if n is None else n, table, nbytes, 1, tau, None), word)
        return arr

    good = [Pair(p, p + 64, 8)]
    polyak(b"null pairs", None, n=1)
    polyak(b"n_pairs must be >= 1", good, n=0)
    polyak(b"numel must be >= 0", [Pair(p, p + 64, -1)])
    polyak(b"null src or dst", [Pair(None, p, 8)])
    polyak(b"null src or dst", good + [Pair(p, None, 8)])
    polyak(b"not 4-B aligned", [Pair(p + 2, p + 64, 8)])
    polyak(b"same address", good + [Pair(p + 32, p + 32, 8)])
    for tau in (-1e-9, 1.0000001, float("nan"), float("inf")):
        polyak(b"tau must be in [0, 1]", good, tau=tau)
    polyak(b"null table", good, table=None)
    polyak(b"not 8-B aligned", good, table=p + 4)
    polyak(b"too small", good, nbytes=31)
    # the table: 24 B per pair that holds elements, 8 B per chunk of C; zero-element pairs are skipped, unread
    arr = (Pair * 3)(Pair(p, p + 64, 2 * S.C + 3), Pair(None, None, 0), Pair(p, p + 64, 1))
    assert lib.usv_polyak_table_bytes(arr, 3) == 2 * 24 + (3 + 1) * 8
    assert lib.usv_polyak_table_bytes(arr, 0) == 0
    none = (Pair * 1)(Pair(None, None, 0))
    assert lib.usv_polyak_update(none, 1, None, 0, 1, 0.005, None) == 0      # nothing to do: no launch


def test_polyak_of_empty_pairs_alone_needs_no_device(lib):
    """A list whose every pair has numel == 0 is USV_OK before any HIP call: neither the pointers nor the table are
    looked at."""
    from gym_usv_amd import _lib
    Pair = _lib.UsvPolyakPair
    for n in (1, 3, 130):
        arr = (Pair * n)(*(Pair(None if i % 2 else 8, None if i % 3 else 2, 0) for i in range(n)))
        assert lib.usv_polyak_table_bytes(arr, n) == 0
        for tau in (0.0, 0.005, 1.0):
            assert lib.usv_polyak_update(arr, n, None, 0, 1, tau, None) == 0, (n, tau, lib.usv_last_error())


def test_python_checks_need_no_device():
    import torch
    import gym_usv_amd
    from gym_usv_amd import sac
    assert gym_usv_amd.DeviceSACLoss is sac.DeviceSACLoss and gym_usv_amd.DevicePolyak is sac.DevicePolyak
    assert gym_usv_amd.CriticLoss._fields == ("loss", "target")
    assert gym_usv_amd.PolicyLoss._fields == ("actor_loss", "ent_coef_loss")
    with pytest.raises(gym_usv_amd.UsvLibError):
        sac.DeviceSACLoss(torch.device("cpu"))
    ent, rows = torch.ones(1), torch.zeros(4)
    grad_ent = torch.ones(1, requires_grad=True)
    for kw in (dict(ent_coef=ent, logp_next=None, discounts=None, gamma=0.99),
               dict(ent_coef=None, logp_next=rows, discounts=None, gamma=0.99),
               dict(ent_coef=ent, logp_next=rows, discounts=None, gamma=None),
               dict(ent_coef=ent, logp_next=rows, discounts=rows, gamma=0.99),
               dict(ent_coef=grad_ent, logp_next=rows, discounts=rows, gamma=None)):
        with pytest.raises(ValueError):
            sac.check_critic_args(**kw)
    assert sac.check_critic_args(ent, rows, rows, None) == 0.0 and sac.check_critic_args(None, None, None, 0.5) == 0.5
    for a in ((grad_ent, None, None), (0.2, None, None), (ent, grad_ent, None), (ent, None, -2.0)):
        with pytest.raises(ValueError):
            sac.check_policy_args(*a)
    assert sac.check_policy_args(ent, grad_ent, -2) == -2.0
    for bad in (torch.zeros(4, dtype=torch.float64), torch.zeros(4, 2), torch.zeros(0), torch.zeros(5), 3.0):
        with pytest.raises(ValueError):
            sac._rows("q2", bad, 4)
    assert sac._rows("q2", torch.zeros(4, 1), 4).shape == (4, 1)
    a, b = torch.zeros(3, 4), torch.zeros(3, 4)
    for params, targets in (([a], [b, b]), ([], []), ([a.double()], [b]), ([a], [b.double()]), ([a.t()], [b.t()]),
                            ([a], [torch.zeros(4, 3)]), ([a], [torch.zeros(12)])):
        with pytest.raises(ValueError):
            sac.DevicePolyak(params, targets)
    with pytest.raises(gym_usv_amd.UsvLibError):          # well-formed, but not on a GPU: no CPU fallback
        sac.DevicePolyak([a], [b])
