"""Synthetic Tanner graphs with prescribed node degrees, for the tests that walk the whole degree envelope of the C ABI (checks of
degree 2-8, variables of degree 1-8): the generator, the degree profiles, and the reference-format code file of such a graph."""
import numpy as np

QS = (4, 8, 16, 32, 64, 128, 256)

# id -> (check degrees, variable degrees, degrees that exactly one variable has)
PROFILES = {
    "dc2": ((2,), (2,), ()),                                # no interior edge; general check-node kernels only
    "dc2mix": ((2, 3, 4), (2, 3), ()),                      # one degree-2 check makes the specialised kernels step aside
    "dc78": ((7, 8), (2, 3), ()),                           # largest checks under the fused small-field iteration
    "dv48": ((4, 5), (4, 5, 6, 7, 8), ()),                  # separate variable-node launch, eight c2v vectors per variable
    "dv4edge": ((3, 4), (2, 3), (4,)),                      # upper side of the fused / unfused switch: ONE variable of degree 4
    "all": ((2, 3, 4, 5, 6, 7, 8), (1, 2, 3, 4, 5, 6, 7, 8), ()),
}
# the T-EMS trellis path code is one 32-bit word: log2(q) * maxdc <= 32 (nbl_create refuses the rest).  At GF(128) / GF(256) the
# T-EMS cells of dv48 run with checks of degree 3 and 4 (7 * 5 and 8 * 5 bits do not fit; the variable side is what dv48 is about).
TEMS_CHK_DEGS = {("dv48", 128): (3, 4), ("dv48", 256): (3, 4)}
# (profile, q) whose T-EMS decoder nbl_create must refuse -- every other (profile, q, method) cell runs
TEMS_REFUSED = [(prof, q) for prof in ("dc78", "all") for q in (32, 64, 128, 256)]


def profile_degrees(profile, q=None, method=None):
    chk, var, once = PROFILES[profile]
    if method == "tems":
        chk = TEMS_CHK_DEGS.get((profile, q), chk)
    return chk, var, once


def _fill(total, degs):
    """Fewest degrees out of `degs` (repeats allowed) that sum to `total`, or None."""
    best = {0: []}
    for s in range(1, total + 1):
        c = [best[s - d] + [d] for d in degs if s - d in best]
        if c:
            best[s] = min(c, key=len)
    return best.get(total)


def degree_code(q, seed, chk_degs, var_degs, M, once=()):
    """Graph with M checks whose degrees cycle through `chk_degs` and variables whose degrees cycle through `var_degs` (after
    one variable for every degree in `once`; the last few degrees are whatever of `var_degs` uses up the sockets).  Sockets of
    the checks are shuffled and handed to the variables (largest first, so that a degree-8 variable still finds eight different
    checks), skipping the checks a variable has already joined; a dead end starts over with the next shuffle of the same seeded
    stream.  No variable joins a check twice.  Non-zero coefficients from the seed; variables in a seeded random order, so that
    long and short ones sit side by side.  The realised degree sets are asserted to be the requested ones.
    Returns (nb.Code, oracle edge tuple, spec); the check-major edge order is the one the oracle derives from the variable-major
    list (a check lists its variables by increasing index)."""
    import nbldpc_amd as nb
    rng = np.random.default_rng(seed)
    cdeg = [chk_degs[m % len(chk_degs)] for m in range(M)]
    S = sum(cdeg)
    vdeg, k = list(once), 0
    while sum(vdeg) + var_degs[k % len(var_degs)] <= S - 2 * max(var_degs):
        vdeg.append(var_degs[k % len(var_degs)])
        k += 1
    tail = _fill(S - sum(vdeg), [d for d in var_degs if d not in once])
    assert tail is not None, (chk_degs, var_degs, M)
    vdeg += tail
    assert max(vdeg) <= M
    rows = None
    for _ in range(2000):
        sockets = [m for m in range(M) for _ in range(cdeg[m])]
        rng.shuffle(sockets)
        rows = []
        for d in sorted(vdeg, reverse=True):
            pick = []
            for i, m in enumerate(sockets):
                if m not in [sockets[j] for j in pick]:
                    pick.append(i)
                    if len(pick) == d:
                        break
            if len(pick) < d:
                rows = None
                break
            rows.append(sorted(sockets[j] for j in pick))
            sockets = [m for i, m in enumerate(sockets) if i not in pick]
        if rows is not None:
            break
    assert rows is not None, "no simple graph found for this degree sequence"
    rows = [rows[i] for i in rng.permutation(len(rows))]
    N = len(rows)
    var_rows = [[(m + 1, int(rng.integers(1, q))) for m in r] for r in rows]
    chk_rows = [[] for _ in range(M)]
    ev, ec, eh = [], [], []
    for n, r in enumerate(var_rows):
        for m1, h in r:
            chk_rows[m1 - 1].append((n + 1, h))
            ev.append(n); ec.append(m1 - 1); eh.append(h)
    spec = dict(N=N, M=M, q=q, var_rows=var_rows, chk_rows=chk_rows)
    code = nb.Code(spec=spec)
    assert sorted(set(code.chk_deg.tolist())) == sorted(set(chk_degs)), (sorted(set(code.chk_deg.tolist())), chk_degs)
    assert sorted(set(code.var_deg.tolist())) == sorted(set(var_degs) | set(once)), (sorted(set(code.var_deg.tolist())), var_degs, once)
    for d in once:
        assert int((code.var_deg == d).sum()) == 1, (d, code.var_deg.tolist())
    return code, (N, M, q, np.array(ev, np.int32), np.array(ec, np.int32), np.array(eh, np.int32)), spec


def profile_code(profile, q, method=None, M=None, seed=None):
    """The graph of one (profile, q) cell: M = 14 checks ('all': every check degree twice), 12 otherwise."""
    chk, var, once = profile_degrees(profile, q, method)
    if M is None:
        M = 14 if profile == "all" else 12
    if seed is None:
        seed = 7000 + 10 * q + sorted(PROFILES).index(profile) + (5 if chk != PROFILES[profile][0] else 0)
    return degree_code(q, seed, chk, var, M, once=once)


def spec_edges(spec):
    """(nb.Code, oracle edge tuple) of a graph spec stored in a fixture's meta."""
    import nbldpc_amd as nb
    ev, ec, eh = [], [], []
    for n, r in enumerate(spec["var_rows"]):
        for m1, h in r:
            ev.append(n); ec.append(m1 - 1); eh.append(h)
    return nb.Code(spec=spec), (spec["N"], spec["M"], spec["q"], np.array(ev, np.int32), np.array(ec, np.int32), np.array(eh, np.int32))


def write_spec_code_file(spec, path):
    """The parity-check file of a graph spec, in the layout nbldpc_amd/datafiles.py::write_code_file writes for a shipped code."""
    lines = [f"{spec['N']} {spec['M']} {spec['q']}",
             f"{max(len(r) for r in spec['var_rows'])} {max(len(r) for r in spec['chk_rows'])}",
             " ".join(str(len(r)) for r in spec["var_rows"]) + " ",
             " ".join(str(len(r)) for r in spec["chk_rows"]) + " "]
    for row in spec["var_rows"] + spec["chk_rows"]:
        lines.append(" ".join(f"{a} {h}" for a, h in row) + " ")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path


def ring_code(q, M, dc):
    """A synthetic (2, dc)-regular graph (dc even): M checks, N = M dc / 2 variables; variable n joins checks n % M and
    (n % M + 1 + n // M) % M -- two different checks, every check gets dc / 2 variables from each rule."""
    assert dc % 2 == 0 and M > dc // 2
    N = M * dc // 2
    chk_rows = [[] for _ in range(M)]
    var_rows = [[] for _ in range(N)]
    for n in range(N):
        for m in (n % M, (n % M + 1 + n // M) % M):
            h = 1 + (7 * n + 3 * m) % (q - 1)
            var_rows[n].append((m + 1, h))
            chk_rows[m].append((n + 1, h))
    import nbldpc_amd as nb
    return nb.Code(spec=dict(N=N, M=M, q=q, var_rows=var_rows, chk_rows=chk_rows))
