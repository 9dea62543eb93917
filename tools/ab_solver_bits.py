"""Bit identity of the solver's entries and of a short solve between two builds of the library.
Usage: python tools/ab_solver_bits.py LIB_A LIB_B [--out DIR]

One fresh child process per library (SFMBA_LIB), each under its own time limit; the tool stops at the first child that
does not exit cleanly.  A child runs normal_blocks, rhs_precond, schur_matvec and step_products, then one solve of
five function evaluations, on the hand-built problem of tests/entry_bounds.py.  It does so in 64- and in 32-bit storage for every option set
of that file's case tables and of tests/entry_bounds32.py's (cam_chunk, rhsrec, xcd_chunks, xcd_cam, pcg_mixed,
pcg_mixed_b, and sweep_rc / vec_lds, which also decide pcg_fused and round_blocks) and with precond = 0, and writes every returned array to
DIR/solver_bits_<a|b>.npz (DIR: a fresh temporary folder unless --out names one).  An entry that a form refuses
(rhs_precond on stored fp32 blocks; step_products in 32-bit storage by a library older than its fp32 form, against which
the newer one then shows those arrays as differing) is recorded by its message and listed in the report.
The parent compares the two files byte for byte."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "sfm-python_amd"), os.path.join(ROOT, "tests")]
import numpy as np

CHILD_SECONDS = 400


def cases():
    """(tag, bits, debug options) of every row of the case tables that runs on the hand-built problem, each once."""
    import entry_bounds as eb
    import entry_bounds32 as eb32
    seen = set()
    for table in (eb.BLOCK_CASES, eb.RHS_CASES, eb.SCHUR_CASES, eb32.MIXED_CASES, eb32.STORED_CASES):
        for row in table.values():
            if row[0] == "hand_built":
                options = next(v for v in row[1:] if isinstance(v, dict))
                for bits in (64, 32):                             # (the 32-bit tests run the 64-bit tables too)
                    seen.add((bits, tuple(sorted(options.items()))))
    for bits in (64, 32):                                         # rhs without the preconditioner: k_cam_schur<1, *>
        seen.update({(bits, (("precond", 0),)), (bits, (("precond", 0), ("sweep_rc", 0)))})
    seen.add((64, (("rc_consumers", 1),)))                        # k_jdot_rc, k_backsub_rc: step_products and the solve
    for bits in (64, 32):                                         # k_jdot<false, true>, k_backsub<false, true>
        seen.add((bits, (("jfree", 1),)))
    for bits, options in sorted(seen):
        yield f"{bits}|" + (",".join(f"{k}={v}" for k, v in options) or "default"), bits, dict(options)


def child(out_path):
    import sfmba
    import entry_bounds as eb
    from oracle import ba_oracle as orc
    args, x = eb.problem("hand_built", orc)
    lin = eb.linearisation("hand_built", orc)
    dc, dp, v = eb.operands(lin, eb.structure("hand_built", orc, {}))
    sg = np.random.default_rng(3).normal(size=x.shape[0])
    out = {}
    for tag, bits, options in cases():
        be = sfmba.Backend(0)
        be.set_precision(bits)
        be.debug_option("dense", 0)
        for name, value in options.items():
            be.debug_option(name, value)
        be.set_problem(*args)
        entries = (("blocks", ("U", "V", "gc", "gp"), lambda: be.normal_blocks(x)),
                   ("rhs", ("rhs", "sd", "minv"), lambda: be.rhs_precond(x, dc, dp)),
                   ("schur", ("y",), lambda: (be.schur_matvec(x, dc, dp, v),)),
                   ("step", None, lambda: be.step_products(x, sg, dc, dp)))
        def solve():
            opt = be.default_options()
            opt.max_nfev = 5
            xs, res, fun, grad = be.solve(x, opt)
            return {"x": xs, "fun": fun, "grad": grad, "scalars": np.array([res.nfev, res.cost], dtype=np.float64),
                    "pcg": np.asarray(be.pcg_history(), dtype=np.int64)}
        entries += (("solve", None, solve),)
        for what, fields, call in entries:
            try:
                got = call()
            except ValueError as e:                              # an entry that this storage mode or form does not offer:
                out[f"{tag}|{what}|refused"] = np.frombuffer(str(e).encode(), dtype=np.uint8)     # the refusal is compared
                continue
            for f, a in (got.items() if fields is None else zip(fields, got)):
                out[f"{tag}|{what}|{f}"] = np.asarray(a)
        be.close()
    np.savez(out_path, **out)


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--child"]:
        return child(argv[1])
    out_dir = None
    if "--out" in argv:
        k = argv.index("--out")
        out_dir = argv[k + 1]
        del argv[k:k + 2]
    lib_a, lib_b = (os.path.abspath(p) for p in argv)
    if out_dir is None:
        out_dir = tempfile.mkdtemp(prefix="solver_bits_")
    os.makedirs(out_dir, exist_ok=True)
    files = []
    for tag, lib in (("a", lib_a), ("b", lib_b)):
        path = os.path.join(out_dir, f"solver_bits_{tag}.npz")
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=dict(os.environ, SFMBA_LIB=lib),
                                timeout=CHILD_SECONDS).returncode
        except subprocess.TimeoutExpired:
            rc = "time limit"
        if rc != 0:
            print(f"{lib}: the child ended with {rc}; stopping")
            return 2
        files.append(np.load(path))
    a, b = files
    print(f"A = {lib_a}\nB = {lib_b}")
    differ = [k for k in a.files if k not in b.files or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
    differ += [k for k in b.files if k not in a.files]
    groups = {}
    for k in a.files:
        g = "/".join(k.split("|")[:2])
        n, bad = groups.get(g, (0, 0))
        groups[g] = (n + 1, bad + (k in differ))
    for g, (n, bad) in groups.items():
        print(f"  {g:48s} {n:4d} arrays  {'identical' if not bad else '%d DIFFER' % bad}")
    nbytes = sum(a[k].nbytes for k in a.files)
    print(f"{len(a.files)} arrays, {nbytes} bytes: " + ("every array identical" if not differ else f"{len(differ)} arrays differ"))
    for k in differ[:20]:
        print("  differs:", k.replace("|", "/"))
    for k in a.files:
        if k.endswith("|refused"):
            print("  refused:", k.replace("|", "/")[:-8], "--", a[k].tobytes().decode())
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
