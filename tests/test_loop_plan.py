"""The host's decisions in the iteration loops (csrc/ofx_loop_plan.h), pinned without a GPU: tests/loop_plan_driver.cpp is built with
the host C++ compiler against the header alone and prints the rules over grids; every line is compared with a restatement below.
The restatements are the code these rules had while every loop runner and every solver driver carried a copy of its own: the
chunk loop, the "ended inside a unit" test and the took_alt rule of ofx_run_loop_group, the b0 / code / nit / redo / result
expressions of the seven drivers (three TV-L1, HS, Brox and temporal-Brox tiles) and tvl1_pick_rows2 / tvl1_pick_rows3.  The pump
runs against a scripted device (polls complete in order, pair g stops at n_g) and must issue what the old runner issued."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "optical-flow-1_amd", "csrc")
FS = (1, 2, 3, 4, 6)
MAXES = tuple(range(1, 25)) + (300,)


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def driver():
    out = os.path.join(HERE, "_build", "loop_plan_driver")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC,
           os.path.join(HERE, "loop_plan_driver.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def lines(driver, what):
    r = subprocess.run([driver, what], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [ln for ln in r.stdout.split("\n") if ln]


# ---- the loop rules -------------------------------------------------------------------------------------------------------------

def old_schedule(max_iter, F, chunk):
    """the enqueueing loop ofx_run_loop_group had, with nothing to stop it: [(launches of a chunk, (first, launched))]"""
    chunk = 1 if chunk < 1 else chunk
    chunk = (chunk + F - 1) // F * F
    launched, out = 0, []
    while launched < max_iter:
        first = launched
        c = max_iter - launched if max_iter - launched < chunk else chunk
        ls = []
        while launched < first + c:
            cnt = first + c - launched if first + c - launched < F else F
            ls.append((launched, cnt))
            launched += cnt
        out.append((ls, (first, launched)))
    return out


def old_inside(n, F, max_iter):
    """(r, k0, cnt) of the redo decision"""
    k0 = (n - 1) // F * F
    cnt = max_iter - k0 if max_iter - k0 < F else F
    return (F > 1 and n > 0 and n - k0 != cnt), k0, cnt


@pytest.fixture(scope="module")
def loop_lines(driver):
    return lines(driver, "loop")


def test_chunk_schedule_and_poll_ranges(loop_lines):
    seen = set()
    for ln in loop_lines:
        if not ln.startswith("sched"):
            continue
        head, body = ln.split(":")
        _, max_iter, F, chunk = head.split()
        max_iter, F, chunk = int(max_iter), int(F), int(chunk)
        got, ls = [], []
        for tok in body.split():
            if tok[0] == "[":
                a, b = tok[1:-1].split(",")
                got.append((ls, (int(a), int(b))))
                ls = []
            else:
                k, cnt = tok.split("+")
                ls.append((int(k), int(cnt)))
        assert got == old_schedule(max_iter, F, chunk), ln
        flat = [kc for ls, _ in got for kc in ls]
        assert all(k % F == 0 for k, _ in flat), ln                           # every unit starts at a multiple of F
        assert all(cnt == F for _, cnt in flat[:-1]), ln
        k0, cnt = flat[-1]
        assert cnt == max_iter - k0 and 1 <= cnt <= F, ln                     # the last unit is what is left of max_iter
        assert got[0][1][0] == 0 and got[-1][1][1] == max_iter, ln
        assert all(a[1][1] == b[1][0] for a, b in zip(got, got[1:])), ln      # the poll ranges tile [0, max_iter)
        seen.add((max_iter, F, chunk))
    assert seen == {(m, F, c) for m in MAXES for F in FS for c in range(1, 14)}


def test_units_inside_and_redo_entries(loop_lines):
    seen = set()
    for ln in loop_lines:
        if not ln.startswith("unit"):
            continue
        max_iter, F, n, k0, cnt, inside, unit, count, ran = map(int, ln.split()[1:])
        r, k0_old, cnt_old = old_inside(n, F, max_iter)
        assert (k0, cnt, bool(inside)) == (k0_old, cnt_old, r), ln
        assert k0 % F == 0 and k0 < n <= k0 + cnt <= max_iter, ln
        assert bool(inside) == (n != k0 + cnt), ln                            # exactly when n is not its unit's last iteration
        if F == 2:
            assert bool(inside) == (n % 2 == 1 and n != max_iter), ln
        j = (n - 1) // F                                                      # the redo lambdas: n = k_of + 1, j = (n - 1) / K, n - j K
        assert (unit, count) == (j, n - j * F) and 1 <= count <= F, ln
        assert ran == (n + F - 1) // F, ln                                    # the epilogues
        seen.add((max_iter, F, n))
    assert seen == {(m, F, n) for m in MAXES for F in FS for n in range(1, m + 1)}


def test_took_alt(loop_lines):
    count = 0
    for ln in loop_lines:
        if not ln.startswith("alt"):
            continue
        max_iter, F, n, wants, apred, abit, value = map(int, ln.split()[1:])
        r = old_inside(n, F, max_iter)[0]
        stored = r and F == 2 and bool(wants) and (bool(apred) or (n == 1 and bool(abit)))
        assert bool(value) == stored, ln
        count += 1
    assert count == 8 * sum(MAXES) * len(FS)


# ---- the pump ---------------------------------------------------------------------------------------------------------------------

def old_group_loop(max_iter, F, chunk, max_out, n_of):
    """ofx_run_loop_group as it was, against the scripted device: (stop, trace, [(n, redo_k)])"""
    chunk = 1 if chunk < 1 else chunk
    chunk = (chunk + F - 1) // F * F
    launched = head = tail = 0
    rec, tr, stop, fin = {}, [], False, None
    while True:
        while launched < max_iter and head - tail < max_out:
            first = launched
            c = max_iter - launched if max_iter - launched < chunk else chunk
            while launched < first + c:
                cnt = first + c - launched if first + c - launched < F else F
                tr.append("L%d+%d" % (launched, cnt))
                launched += cnt
            tr.append("P%d,%d" % (first, launched))
            rec[head & 1] = [(n, 1) if 0 < n <= launched else (launched, int(launched >= max_iter)) for n in n_of]
            head += 1
        if tail == head:
            break
        fin = rec[tail & 1]
        all_done = all(d for _, d in fin)
        tail += 1
        tr.append("R1" if all_done else "R0")
        if all_done:
            stop = True
            break
    return stop, tr, [(n, n - 1 if old_inside(n, F, max_iter)[0] else -1) for n, _ in fin]


def test_pump_against_a_scripted_device(driver):
    seen = set()
    for ln in lines(driver, "pump"):
        head, status, trace, ends = ln.split(":")
        nums = list(map(int, head.split()[1:]))
        max_iter, F, chunk, max_out, G, n_of = nums[0], nums[1], nums[2], nums[3], nums[4], nums[5:]
        assert len(n_of) == G
        stop, tr, fin = old_group_loop(max_iter, F, chunk, max_out, n_of)
        assert status.split() == ["0", "1"] and stop, ln
        assert trace.split() == tr, ln
        assert [tuple(map(int, e.split("/"))) for e in ends.split()] == fin, ln
        # what the loop promises, from the trace alone
        sched = old_schedule(max_iter, F, chunk)
        outstanding = polls = 0
        launches = []
        last = max(n if n else max_iter for n in n_of)          # the iteration that ends the last pair's loop
        for i, tok in enumerate(tr):
            if tok[0] == "L":
                launches.append(tuple(map(int, tok[1:].split("+"))))
            elif tok[0] == "P":
                outstanding += 1
                polls += 1
                assert outstanding <= max_out, ln                                # at most max_out polls outstanding
            else:
                outstanding -= 1
                assert outstanding >= 0, ln
                assert (tok == "R1") == (i == len(tr) - 1), ln                   # nothing is launched once "all done" has been read
        flat = [kc for ls, _ in sched for kc in ls]
        assert launches == flat[:len(launches)], ln                              # a prefix of the schedule
        assert launches == [kc for ls, _ in sched[:polls] for kc in ls], ln      # ... in whole chunks
        need = next(i for i, (_, (a, b)) in enumerate(sched) if b >= last) + 1   # chunks up to the one that holds the stop
        assert need <= polls <= min(len(sched), need + max_out), ln              # at most max_out chunks behind the stop
        seen.add((max_iter, F, chunk, max_out, G, n_of[0]))
    assert seen == {(m, F, c, o, G, n) for m in (1, 2, 5, 7, 12, 24) for F in FS for c in (1, 4, 5, 13) for o in (1, 2) for G in (1, 3)
                    for n in range(0, m + 1)}


# ---- the launch-unit table ----------------------------------------------------------------------------------------------------------

def start_buffers(MOD, G, cur):
    bits = 2 if MOD == 3 else 1
    return [(cur >> (bits * g)) & ((1 << bits) - 1) for g in range(G)]


def driver_patterns(G, j):
    """the arguments tests/loop_plan_driver.cpp feeds the table at point j"""
    ran = [(j + g) % 8 for g in range(G)]
    alt = [(g + j) & 1 for g in range(G)]
    k_of = [-1 if g % 3 == 2 else (5 * j + 3 * g) % 24 for g in range(G)]
    u_of = [(j + 2 * g) % 8 for g in range(G)]
    k0_of = [3 * u for u in u_of]
    n_of = [-1 if g % 4 == 1 else k0_of[g] + 1 + (g + j) % 3 for g in range(G)]
    return ran, alt, k_of, n_of, k0_of, u_of


def old_codes(MOD, G, b0, j):
    all_ = (1 << G) - 1
    if MOD == 3:        # the code_of / code_of_unit lambdas the TV-L1 drivers had
        c = 0
        for g in range(G):
            c |= ((b0[g] + j) % 3) << (2 * g)
        return c, all_
    packed = sum(b << g for g, b in enumerate(b0))          # ofx_hs_tile_solve: b0 ^ flip (the Brox tiles: b0 = 0)
    return packed ^ (all_ if (j & 1) else 0), all_


def old_redo(MOD, G, b0, k_of, K):
    incode = runmask = nit = 0
    for g in range(G):
        if k_of[g] < 0:
            continue
        n = k_of[g] + 1
        j = (n - 1) // K
        runmask |= 1 << g
        if MOD == 3:
            incode |= ((b0[g] + j) % 3) << (2 * g)
            if K == 2:
                assert j == k_of[g] // 2                      # the two-iteration driver wrote b0 + k_of / 2
        else:
            incode |= ((b0[g] ^ j) & 1) << g
        nit |= (n - j * K) << (4 * g)
    return incode, runmask, nit


def old_redo_cursor(G, b0, n_of, k0_of, u_of):
    incode = runmask = nit = 0
    for g in range(G):
        if n_of[g] < 0:
            continue
        runmask |= 1 << g
        incode |= ((b0[g] + u_of[g]) % 3) << (2 * g)
        nit |= (n_of[g] - k0_of[g]) << (4 * g)
    return incode, runmask, nit


def old_result(MOD, G, b0, ran, alt):
    c = 0
    for g in range(G):
        if MOD == 3:
            c |= ((b0[g] + ran[g] + (1 if alt and alt[g] else 0)) % 3) << (2 * g)
        else:
            c |= ((b0[g] ^ ran[g]) & 1) << g
    return c


def test_unit_table(driver):
    seen = set()
    for ln in lines(driver, "units"):
        f = ln.split()
        kind, MOD, G, cur, j = f[0], int(f[1]), int(f[2]), int(f[3], 16), int(f[4])
        b0 = start_buffers(MOD, G, cur)
        assert all(b < MOD for b in b0)
        ran, alt, k_of, n_of, k0_of, u_of = driver_patterns(G, j)
        width = (2 if MOD == 3 else 1) * G
        if kind == "code":
            code, all_, nit = int(f[5], 16), int(f[6], 16), int(f[7], 16)
            assert (code, all_) == old_codes(MOD, G, b0, j), ln
            assert nit == sum((j % 6 + 1) << (4 * g) for g in range(G)), ln
            assert code >> width == 0 and all_ >> G == 0 and nit >> (4 * G) == 0, ln
        elif kind == "result":
            plain, with_alt = int(f[5], 16), int(f[6], 16)
            assert plain == old_result(MOD, G, b0, ran, None), ln
            if MOD == 3:
                assert with_alt == old_result(MOD, G, b0, ran, alt), ln
            assert plain >> width == 0 and with_alt >> width == 0, ln
        elif kind == "redo":
            K, got = int(f[5]), tuple(int(x, 16) for x in f[6:9])
            assert got == old_redo(MOD, G, b0, k_of, K), ln
            assert got[0] >> width == 0 and got[1] >> G == 0 and got[2] >> (4 * G) == 0, ln
        else:
            assert kind == "redoc"
            got = tuple(int(x, 16) for x in f[5:8])
            if MOD == 3:
                assert got == old_redo_cursor(G, b0, n_of, k0_of, u_of), ln
            assert got[0] >> width == 0 and got[1] >> G == 0 and got[2] >> (4 * G) == 0, ln
        seen.add((kind, MOD, G, tuple(b0[:2]), j))
    for MOD in (2, 3):
        for G in (1, 2, 16):
            starts = {s[3] for s in seen if s[1] == MOD and s[2] == G}
            assert {b[0] for b in starts} == set(range(MOD))                           # every start buffer, in every position
            if G > 1:
                assert starts == {(a, b) for a in range(MOD) for b in range(MOD)}
            assert {s[4] for s in seen if s[1] == MOD and s[2] == G} == set(range(8))  # unit counts 0 .. 7


# ---- strip heights ----------------------------------------------------------------------------------------------------------------

def old_pick_rows2(nx, ny, G, concurrency, rows_slots):
    strips_pad = cdiv(cdiv(nx, 60), 4) * 4 * G                      # STRIP2_OUT
    rmax, best, best_cost = 24, 24, -1
    if concurrency > 1:
        for r in (1, 2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 20, 24):
            waves = strips_pad * cdiv(ny, r)
            slots = rows_slots if rows_slots > 0 else 1024
            cost = ((waves + slots - 1) // slots) * (r + 5)
            if best_cost < 0 or cost < best_cost:
                best_cost, best = cost, r
        return best
    slots = 1024 * 3                                                # OFX_ITER2_WAVES
    for k in range(1, 5):
        for r in range(1, rmax + 1):
            if strips_pad * cdiv(ny, r) > k * slots:
                continue
            cost = k * (r + 5)
            if best_cost < 0 or cost < best_cost:
                best_cost, best = cost, r
            break
    if best < 3 and strips_pad * cdiv(ny, 3) >= 512:
        best = 3
    return best


def old_pick_rows3(nx, ny, G, N, concurrency, rows_slots, rows3_max=32):
    depth = 2 * N + 1
    strips_pad = cdiv(cdiv(nx, 56), 4) * 4 * G                      # STRIP3_OUT
    rmax, best, best_cost = 32, 32, -1
    if concurrency > 1:
        for r in (2, 3, 4, 5, 6, 8, 10, 12, 14, 16, 20, 24, 28, 32, 36, 40, 48, 54, 64, 72, 80, 96):
            if r > rows3_max:
                break
            waves = strips_pad * cdiv(ny, r)
            slots = rows_slots if rows_slots > 0 else 1024
            cost = ((waves + slots - 1) // slots) * (r + depth)
            if best_cost < 0 or cost < best_cost:
                best_cost, best = cost, r
        return best
    slots = 1024 * 3                                                # OFX_ITER3_WAVES
    for k in range(1, 5):
        for r in range(1, rmax + 1):
            if strips_pad * cdiv(ny, r) > k * slots:
                continue
            cost = k * (r + depth)
            if best_cost < 0 or cost < best_cost:
                best_cost, best = cost, r
            break
    if best < 4 and strips_pad * cdiv(ny, 4) >= 512:
        best = 4
    return best


def test_strip_heights(driver):
    dims = (2, 3, 55, 56, 57, 60, 61, 120, 135, 240, 270, 480, 540, 960, 1080, 1920, 2160, 3840)
    seen = set()
    for ln in lines(driver, "rows"):
        N, nx, ny, G, conc, slots, rows = map(int, ln.split()[1:])
        want = old_pick_rows2(nx, ny, G, conc, slots) if N == 2 else old_pick_rows3(nx, ny, G, N, conc, slots)
        assert rows == want, ln
        seen.add((N, nx, ny, G, conc, slots))
    assert seen == {(N, nx, ny, G, c, s) for N in (2, 3, 4) for nx in dims for ny in dims for G in (1, 2, 5, 16) for c in (1, 4)
                    for s in (0, 512)}


def test_the_library_uses_the_shipping_models():
    """the driver restates two numbers per kernel that ofx_tvl1.hip owns: strip width and resident waves per SIMD"""
    src = open(os.path.join(CSRC, "ofx_tvl1.hip")).read()
    for name, value in (("STRIP2_OUT", 60), ("OFX_ITER2_WAVES", 3), ("STRIP3_OUT", 56), ("OFX_ITER3_WAVES", 3)):
        assert re.search(r"^#define %s %d\b" % (name, value), src, re.M), name
    assert "ofx_strip_model2(STRIP2_OUT, OFX_ITER2_WAVES)" in src and "ofx_strip_model3(N, STRIP3_OUT, OFX_ITER3_WAVES)" in src
