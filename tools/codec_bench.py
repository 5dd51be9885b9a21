"""What the bench scripts under tools/ share: the profile window over a table of kernel cases, one `dxtexconv -timing` run and its
parser, the one-unmeasured-then-`runs` loop over one or two builds, the `run ...` lines of a host test program's time_ commands by field
name, and the two clocks of copyrect_bench.py and single_plane_bench.py. Imports without a GPU: a script makes its own Context."""
import json, os, re, statistics, subprocess, time

TIMING = re.compile(r": ([0-9.]+) ms, host -> device (\d+) bytes, device -> host (\d+) bytes")


def profile_cases(ctx, cases, texels, reps, warm=3):
    """cases: (mark, what, bytes a texel, call). Each call `warm` times, then `reps` times inside one profile window; prints and returns
    one row a case: every kernel's milliseconds a call, and the TB/s of `mark` over texels * bytes a texel."""
    rows = []
    for mark, what, bytes_a_texel, call in cases:
        for _ in range(warm):
            call()
        ctx.synchronize()
        ctx.profile_begin()
        for _ in range(reps):
            call()
        prof = ctx.profile_end()
        row = {"kernel": mark, "case": what}
        for k, (ms, n) in sorted(prof.items()):
            row[k + " ms"] = round(ms / reps, 4)
        row["TBps"] = round(texels * bytes_a_texel / (prof[mark][0] / reps * 1e-3) / 1e12, 3)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def parse_timing(stdout):
    """dxtexconv's -timing line -> (milliseconds, bytes host -> device, bytes device -> host)"""
    m = TIMING.search(stdout)
    assert m, stdout
    return float(m.group(1)), int(m.group(2)), int(m.group(3))


def conv_run(conv, args, out):
    """one `dxtexconv -timing` run that writes `out` afresh -> (milliseconds, bytes up, bytes down, the bytes of `out`)"""
    if os.path.exists(out):
        os.remove(out)
    r = subprocess.run([conv, "-nologo", "-timing", "-overlap", "1", "-y"] + args, capture_output=True, text=True, check=True)
    with open(out, "rb") as f:
        return parse_timing(r.stdout) + (f.read(),)


def measure_conv(cases, builds, runs):
    """cases: (title, dxtexconv arguments, output file); builds: (name or None, dxtexconv path), ours first. One unmeasured run a build (the
    first touch of a file and of the device), then `runs` runs alternating over the builds. Prints and returns one row a case and build, with
    the build's name where it has one; with two builds also whether their outputs are the same bytes and whether ours is slower than the
    other by more than the other's spread."""
    rows = []
    for title, args, result in cases:
        times = {name: [] for name, _ in builds}
        moved, files = {}, {}
        for name, conv in builds:
            conv_run(conv, args, result)
        for _ in range(runs):
            for name, conv in builds:
                ms, up, down, data = conv_run(conv, args, result)
                times[name].append(ms); moved[name] = (up, down); files[name] = data
        for name, _ in builds:
            t = times[name]
            rows.append({"case": title, **({"build": name} if name else {}), "ms": t, "median": statistics.median(t), "spread": round(max(t) - min(t), 1),
                         "host -> device": moved[name][0], "device -> host": moved[name][1]})
            print(json.dumps(rows[-1]), flush=True)
        if len(builds) > 1:
            (ours, _), (other, _) = builds
            print(json.dumps({"case": title, "outputs byte-identical": files[ours] == files[other],
                              "slower than the parent by more than its spread": rows[-2]["median"] > rows[-1]["median"] + rows[-1]["spread"]}), flush=True)
    return rows


SIDES = ("resident", "host")                                                      # "<side> <ms> ms up <bytes> down <bytes>"
TIMES = ("raw", "undo", "undo_gpu", "texels_gpu")                                 # "<name> <ms> ms", wherever it stands
COUNTS = ("file", "coefficients", "rows")                                         # "<name> <bytes>"


def parse_runs(stdout):
    """the `run <i> ...` lines of a host test program -> one dict a line, by field name: "resident" / "host" with "<side> up" / "<side> down"
    for the pair that follows each, the other times and counts under their own names. A line without a time or with a field cut short raises."""
    rows = []
    for line in stdout.splitlines():
        f = line.split()
        if not f or f[0] != "run":
            continue
        row, side, at = {"run": int(f[1])}, None, 2
        f += ["", ""]          # a field cut short reads these and fails its check
        while at < len(f) - 2:
            key = f[at]
            if key in SIDES or key in TIMES:
                if f[at + 2] != "ms":
                    raise ValueError("no milliseconds after %r: %s" % (key, line))
                row[key] = float(f[at + 1])
                side = key if key in SIDES else None
                at += 3
            elif key in ("up", "down") and side:
                row[side + " " + key] = int(f[at + 1])          # int("") raises ValueError
                at += 2
            elif key in COUNTS:
                row[key] = int(f[at + 1])
                at += 2
            else:
                raise ValueError("unknown field %r: %s" % (key, line))
        for s in SIDES:
            if s in row and not (s + " up" in row and s + " down" in row):
                raise ValueError("no bytes after %r: %s" % (s, line))
        if len(row) == 1 or ("resident" in row) != ("host" in row):
            raise ValueError("a field is missing: " + line)
        rows.append(row)
    return rows


def run_rows(cmd):
    """a time_ command of a host test program, as an argument list -> its parsed `run ...` lines"""
    r = subprocess.run(cmd, capture_output=True, text=True, check=True)
    rows = parse_runs(r.stdout)
    assert rows, r.stdout + r.stderr
    return rows


def summary(rows):
    """parsed lines with both sides -> the keys the scripts print for the resident path beside the host path"""
    res, host = [x["resident"] for x in rows], [x["host"] for x in rows]
    return {"resident ms": res, "resident median": statistics.median(res), "resident up/down": [rows[0]["resident up"], rows[0]["resident down"]],
            "host path ms": host, "host path median": statistics.median(host), "host path spread": round(max(host) - min(host), 1),
            "host path up/down": [rows[0]["host up"], rows[0]["host down"]]}


def api_paths(exe, command, file, runs, extra=()):
    """`exe command file runs *extra` -> the resident path beside the same build's host path"""
    rows = run_rows([exe, command, file, str(runs), *extra])
    assert len(rows) == runs, rows
    return summary(rows)


def med_ms(ctx, fn, reps=20, warm=5):
    """median of the library's own event pair (dxtex_ctx_last_kernel_ms) over `reps` calls"""
    for _ in range(warm): fn()
    ctx.synchronize()
    v = []
    for _ in range(reps):
        fn(); ctx.synchronize(); v.append(ctx.last_kernel_ms())
    return float(statistics.median(v))


def wall_ms(ctx, fn, reps=20, warm=5):
    """median of five wall times of `reps` queued calls and one synchronize, per call"""
    for _ in range(warm): fn()
    ctx.synchronize()
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(reps): fn()
        ctx.synchronize()
        t.append((time.perf_counter() - t0) * 1e3 / reps)
    return float(statistics.median(t))
