"""g2o's Levenberg-Marquardt step control without a GPU: the real header (openmavis_amd/csrc/omv_lm.h) in a stand-alone
program built with -ffp-contract=off -fsanitize=address,undefined (tests/cpp/lm_host.cpp), run on scripted traces, against
tests/lm_ref.py bit for bit -- the script supplies every chi2 and scale, so the two cannot drift apart -- and against the
decisions written out below for every branch of optimization_algorithm_levenberg.cpp:61-185."""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import lm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = lm_ref.DBL_MAX
INF, NAN = float("inf"), float("nan")
SCALE1 = 1.0 - 1e-3   # computeScale for which scale + 1e-3 is 1: rho = currentChi - tempChi


class Trace:
    """A script for lm_host and, in step, lm_ref's rows for it."""

    def __init__(self):
        self.lines, self.rows = [], []
        self.new()

    def new(self):
        self.lines.append("new")
        self.s = lm_ref.LmState()
        return self

    def opt(self, max_trials, user_lambda=0.0, max_diagonal=0.0):
        self.lines.append(f"opt {max_trials} {_txt(user_lambda)} {_txt(max_diagonal)}")
        self.max_trials, self.user, self.md, self.iteration = max_trials, user_lambda, max_diagonal, 0
        return self

    def it(self, chi):
        s = self.s
        self.lines.append(f"it {_txt(chi)}")
        lm_ref.begin_iteration(s, self.iteration, chi, lm_ref.lambda_init(self.user, self.md))
        self.iteration += 1
        self.rows.append(dict(kind="it", lam=s.lam, ni=s.ni, cur=s.current_chi, ini=s.ini_chi, qmax=s.qmax, n_bad=s.n_bad))
        return self.rows[-1]

    def tr(self, chi, solved=True, scale=SCALE1):
        s = self.s
        self.lines.append(f"tr {_txt(chi)} {int(solved)} {_txt(scale)}")
        rho, accepted = lm_ref.trial(s, chi, solved, scale)
        nxt = lm_ref.next_step(s, rho, self.max_trials)
        self.rows.append(dict(kind="tr", lam=s.lam, ni=s.ni, cur=s.current_chi, rho=rho, accepted=accepted, next=nxt,
                              qmax=s.qmax, n_bad=s.n_bad))
        return self.rows[-1]


def _txt(v):
    v = float(v)
    return v.hex() if math.isfinite(v) else repr(v)


def _same(bits_hex, v):
    got = struct.unpack("<d", struct.pack("<Q", int(bits_hex, 16)))[0]
    return (math.isnan(got) and math.isnan(v)) or struct.pack("<d", got) == struct.pack("<d", float(v))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """check(trace): the program's lines for the trace's script equal lm_ref's rows in every field."""
    assert shutil.which("g++") is not None
    exe = str(tmp_path_factory.mktemp("lm_host") / "lm_host")
    src = os.path.join(ROOT, "tests", "cpp", "lm_host.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def check(trace):
        r = subprocess.run([exe], input="\n".join(trace.lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        out = r.stdout.strip().split("\n")
        assert len(out) == len(trace.rows)
        for n, (line, row) in enumerate(zip(out, trace.rows)):
            f = line.split()
            assert f[0] == row["kind"], (n, line, row)
            if row["kind"] == "it":
                ok = all(_same(f[1 + i], row[k]) for i, k in enumerate(("lam", "ni", "cur", "ini")))
                ok = ok and (int(f[5]), int(f[6])) == (row["qmax"], row["n_bad"])
            else:
                ok = all(_same(f[1 + i], row[k]) for i, k in enumerate(("lam", "ni", "cur", "rho")))
                ok = ok and (int(f[5]), f[6], int(f[7]), int(f[8])) == (int(row["accepted"]), row["next"], row["qmax"],
                                                                        row["n_bad"])
            assert ok, (n, trace.lines, line, row)
        return trace
    return check


def test_lambda_init(host):
    t = Trace()
    assert t.opt(10, 5.0, 1234.5).it(1.0)["lam"] == 5.0               # a positive user value wins
    assert t.opt(10, 0.0, 1234.5).it(1.0)["lam"] == 1e-5 * 1234.5     # tau * the maximum
    assert t.opt(10, -1.0, 1234.5).it(1.0)["lam"] == 1e-5 * 1234.5    # `> 0`: a negative one does not count
    assert t.opt(10, 0.0, 0.0).it(1.0)["lam"] == 0.0                  # no vertex, or a zero Hessian
    r = t.rows[-1]
    assert (r["ni"], r["cur"], r["ini"], r["qmax"], r["n_bad"]) == (2.0, 1.0, 1.0, 0, 0)
    host(t)


def test_accepted_trials_and_the_three_ranges_of_the_factor(host):
    t = Trace().opt(10, 1.0)
    t.it(10.0)
    r = t.tr(9.0)   # rho = 1: 1 - 1^3 = 0, clamped to 1/3
    assert (r["rho"], r["accepted"], r["next"], r["lam"], r["ni"], r["cur"], r["qmax"]) == (1.0, True, "iteration", 1. / 3., 2.0, 9.0, 1)
    t.it(9.0)
    r = t.tr(6.0)   # rho = 3: the cube is 125, 1 - 125 clamped to 1/3
    assert (r["rho"], r["accepted"], r["next"], r["lam"]) == (3.0, True, "iteration", 1. / 3. * (1. / 3.))
    t.it(6.0)
    lam = t.s.lam
    r = t.tr(6.0 - 1e-9 * 6.0, scale=6.0 - 1e-3)   # rho = 1e-9: 1 - (-1)^3 = 2, clamped to 2/3 (and a gain under 0.1 %)
    assert 0.9e-9 < r["rho"] < 1.1e-9 and r["accepted"] and r["next"] == "iteration" and r["n_bad"] == 1
    assert r["lam"] == lam * (2. / 3.)
    t.it(r["cur"])
    lam = t.s.lam
    r = t.tr(r["cur"] - 0.9)   # rho = 0.9: 1 - 0.8^3 = 0.488, between the clamps
    a = 2 * r["rho"] - 1
    assert abs(r["rho"] - 0.9) < 1e-12 and r["accepted"] and 1. / 3. < 1. - a * a * a < 2. / 3.
    assert r["lam"] == lam * (1. - a * a * a) and abs(r["lam"] / lam - 0.488) < 1e-12
    host(t)


def test_rejections_double_ni_and_an_accepted_trial_resets_it(host):
    t = Trace().opt(10, 1.0)
    t.it(10.0)
    lams, nis = [], []
    for k in range(4):
        r = t.tr(11.0 + k)   # worse: rho = -1, -2, ...
        assert (r["rho"], r["accepted"], r["next"], r["cur"], r["qmax"]) == (-1.0 - k, False, "trial", 10.0, k + 1)
        lams.append(r["lam"]), nis.append(r["ni"])
    assert nis == [4.0, 8.0, 16.0, 32.0] and lams == [2.0, 8.0, 64.0, 1024.0]   # lambda *= 2, 4, 8, 16
    r = t.tr(9.0)
    assert (r["accepted"], r["ni"], r["lam"], r["next"], r["qmax"]) == (True, 2.0, 1024.0 / 3., "iteration", 5)
    t.it(9.0)
    r = t.tr(9.5)
    assert (r["accepted"], r["ni"], r["lam"]) == (False, 4.0, 1024.0 / 3. * 2.0)   # from 2 again
    host(t)


def test_failed_solve_infinite_and_nan_chi2(host):
    t = Trace().opt(10, 1.0)
    t.it(10.0)
    r = t.tr(5.0, solved=False, scale=2.0)   # tempChi = DBL_MAX over a positive scale: rejected, whatever the chi2
    assert r["rho"] < 0 and (r["accepted"], r["next"], r["lam"], r["ni"], r["cur"]) == (False, "trial", 2.0, 4.0, 10.0)
    r = t.tr(INF, scale=2.0)   # rho = -inf
    assert (r["rho"], r["accepted"], r["next"], r["lam"], r["ni"]) == (-INF, False, "trial", 8.0, 8.0)
    r = t.tr(NAN, scale=2.0)   # no acceptance, the trials end (rho < 0 is false), the optimisation goes on
    assert math.isnan(r["rho"]) and (r["accepted"], r["next"], r["lam"], r["ni"], r["cur"], r["qmax"]) == \
        (False, "iteration", 64.0, 16.0, 10.0, 3)
    assert r["n_bad"] == 1   # no gain in this iteration
    t.it(10.0)
    # a failed solve over a scale below -1e-3: rho > 0 and DBL_MAX is finite, so the reference accepts it
    r = t.tr(5.0, solved=False, scale=-1.0)
    assert r["rho"] > 0 and (r["accepted"], r["cur"], r["lam"], r["ni"], r["next"]) == (True, DBL_MAX, 64.0 / 3., 2.0, "iteration")
    assert r["n_bad"] == 2
    host(t)


def test_equal_chi2_stops(host):
    t = Trace().opt(10, 1.0)
    t.it(10.0)
    r = t.tr(10.0)   # rho == 0: not `> 0`, so rejected, and Terminate
    assert (r["rho"], r["accepted"], r["next"], r["lam"], r["ni"], r["n_bad"]) == (0.0, False, "stop", 2.0, 4.0, 0)
    host(t)


@pytest.mark.parametrize("max_trials", [1, 3, 10])
def test_the_last_allowed_trial_stops(host, max_trials):
    t = Trace().opt(max_trials, 1.0)
    t.it(10.0)
    for k in range(max_trials):
        r = t.tr(11.0)
        assert (r["accepted"], r["qmax"]) == (False, k + 1)
        assert r["next"] == ("stop" if k + 1 == max_trials else "trial"), k
    assert r["ni"] == 2.0 ** (max_trials + 1) and r["n_bad"] == 0   # Terminate comes before the nBad rule
    if max_trials == 1:   # an accepted first trial is the last allowed one as well
        t.new().opt(1, 1.0).it(10.0)
        r = t.tr(9.0)
        assert (r["accepted"], r["next"], r["cur"], r["n_bad"]) == (True, "stop", 9.0, 0)
    else:   # accepted on the last allowed trial: still Terminate
        t.new().opt(max_trials, 1.0).it(10.0)
        for k in range(max_trials - 1):
            assert t.tr(11.0)["next"] == "trial"
        r = t.tr(9.0)
        assert (r["accepted"], r["next"]) == (True, "stop")
    host(t)


def test_three_small_gains_in_a_row_stop_and_a_good_one_between_does_not(host):
    t = Trace().opt(10, 1.0)
    chi, nexts = 1000.0, []
    for k in range(3):   # each gains 0.05 %
        t.it(chi)
        r = t.tr(chi * (1 - 5e-4), scale=chi)
        chi = r["cur"]
        assert r["accepted"] and r["n_bad"] == k + 1
        nexts.append(r["next"])
    assert nexts == ["iteration", "iteration", "stop"]
    t.new().opt(10, 1.0)
    chi, nexts, bads = 1000.0, [], []
    for gain in (5e-4, 5e-4, 2e-3, 5e-4, 5e-4):   # the third gains 0.2 %
        t.it(chi)
        r = t.tr(chi * (1 - gain), scale=chi)
        chi = r["cur"]
        nexts.append(r["next"]), bads.append(r["n_bad"])
    assert nexts == ["iteration"] * 5 and bads == [1, 2, 0, 1, 2]
    # the same state in a second optimize(): iteration 0 resets lambda, ni and nBad
    t.it(chi)
    assert t.tr(chi + 1.0, scale=chi)["next"] == "trial"
    assert (t.s.n_bad, t.s.ni, t.s.qmax) == (2, 4.0, 1) and t.s.lam != 7.0
    r = t.opt(10, 7.0).it(chi)
    assert (r["lam"], r["ni"], r["n_bad"], r["qmax"]) == (7.0, 2.0, 0, 0)
    r = t.tr(chi * (1 - 5e-4), scale=chi)
    assert (r["next"], r["n_bad"]) == ("iteration", 1)
    r = t.it(r["cur"])   # iteration 1 resets nothing
    assert (r["n_bad"], r["lam"], r["ni"]) == (1, t.s.lam, 2.0) and r["lam"] != 7.0
    host(t)


def test_random_traces(host):
    """1,000 seeded traces of up to 10 iterations, drawn so that every decision is common."""
    rng = np.random.default_rng(20261021)
    t = Trace()
    for _ in range(1000):
        user = 0.0 if rng.random() < 0.5 else float(10.0 ** rng.uniform(-9, 3))
        t.new().opt(int(rng.choice([1, 3, 10, 10])), user, float(10.0 ** rng.uniform(-3, 8)))
        chi = float(10.0 ** rng.uniform(-2, 6))
        for _it in range(10):
            t.it(chi)
            while True:
                cur, kind = t.s.current_chi, rng.random()
                rho = float(10.0 ** rng.uniform(-4, 0.5))   # aimed at; the 1e-3 moves it
                if kind < 0.40:     # better
                    temp = cur * (1.0 - float(10.0 ** rng.uniform(-5, -0.3)))
                    r = t.tr(temp, True, (cur - temp) / rho)
                elif kind < 0.80:   # worse
                    temp = cur * (1.0 + float(10.0 ** rng.uniform(-5, 1)))
                    r = t.tr(temp, True, (temp - cur) / rho)
                elif kind < 0.84:
                    r = t.tr(cur, True, float(rng.uniform(0.1, 10)))   # rho == 0
                elif kind < 0.90:
                    r = t.tr(cur * 0.5, False, float(rng.uniform(-3, 3)))   # a failed solve
                elif kind < 0.95:
                    r = t.tr(float(rng.choice([INF, -INF, NAN])), True, float(rng.uniform(0.1, 10)))
                else:               # a negative scale
                    r = t.tr(cur * float(rng.uniform(0.5, 1.5)), True, -float(10.0 ** rng.uniform(-4, 2)))
                if r["next"] != "trial":
                    break
            if r["next"] == "stop":
                break
            chi = r["cur"] if math.isfinite(r["cur"]) and r["cur"] < 1e300 else float(10.0 ** rng.uniform(-2, 6))
    steps = [r for r in t.rows if r["kind"] == "tr"]
    n = len(steps)
    share = dict(accept=sum(r["accepted"] for r in steps) / n, reject=sum(not r["accepted"] for r in steps) / n,
                 retry=sum(r["next"] == "trial" for r in steps) / n, iteration=sum(r["next"] == "iteration" for r in steps) / n,
                 stop=sum(r["next"] == "stop" for r in steps) / n)
    assert n > 5000 and min(share.values()) >= 0.05, (n, share)
    host(t)


def test_product_cube_against_pow():
    """The clamped factor with a * a * a against the reference's pow(a, 3): at most 2^-51 relative apart (the product
    rounds twice where pow rounds once, then 1 - x; measured 3.4e-16 at most over 5 million rho)."""
    rng = np.random.default_rng(7)
    rhos = np.concatenate([rng.uniform(0.84, 0.95, 200000),               # the band where the factor is not clamped
                           10.0 ** rng.uniform(-12, 3, 100000), rng.uniform(0, 2, 100000),
                           [0.5, 1.0, 0.9, 1e-9, 0.7937005259840998, 0.8466]])
    worst, unclamped, differ = 0.0, 0, 0
    for rho in rhos.tolist():
        f = lm_ref.good_step_factor(rho)
        g = max(1. / 3., min(1. - math.pow(2 * rho - 1, 3), 2. / 3.))
        unclamped += 1. / 3. < g < 2. / 3.
        differ += f != g
        worst = max(worst, abs(f - g) / g)
    assert unclamped > 150000
    assert worst <= 2.0 ** -51, (worst, differ)
