"""In-tree build of libpaac_hip.so (gfx950 only).  Used by __graft_entry__.build() and `python -m paac_amd.build`."""
import fcntl
import hashlib
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libpaac_hip.so")
SOURCES = ["api.hip", "net_fwd.hip", "net_bwd.hip", "misc.hip", "games.hip", "optim.hip"]
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join("..", "..", "include", "paac_hip.h")]
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wall", "-Wno-unused-function",
         "-Wno-unused-variable", "-Wno-unused-but-set-variable"]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def library_is_current(lib, extra_deps=()):
    """True where `lib` exists and is newer than every source, every header and this file (and extra_deps: a user game's
    header): nothing it was built from has changed since, whether or not its object files are still there."""
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.abspath(__file__)] + list(extra_deps)
    return not _stale(lib, deps)


def build(force=False, verbose=True, extra_flags=(), lib_path=None, obj_suffix="", extra_deps=(), only=None):
    """extra_flags / lib_path / obj_suffix: diagnostic variants (e.g. -DPAAC_DMM_STAMPS into libpaac_hip_stamps.so).
    extra_deps: files outside csrc/ the variant's objects are built from as well (a user game's header).  only: the sources
    the variant compiles for itself; the others are linked from the stock build's objects, which the caller has made current
    and keeps from being rewritten (build_user_game).
    Safe to call from several processes at once (every torchrun rank calls it for a user architecture): the build runs
    under an exclusive file lock next to the library, objects and library are written to temporary names and renamed into
    place, so a rank that has already loaded the library never sees it rewritten under it."""
    lib = lib_path or LIB
    with open(lib + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            return _build_locked(force, verbose, extra_flags, lib, obj_suffix, extra_deps, only)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _build_locked(force, verbose, extra_flags, lib, obj_suffix, extra_deps=(), only=None):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)] + list(extra_deps)
    objs, jobs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        if only is not None and src not in only:
            objs.append(os.path.join(CSRC, src.replace(".hip", ".o")))      # the stock build's object
            continue
        o = os.path.join(CSRC, src.replace(".hip", obj_suffix + ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append([hipcc] + FLAGS + list(extra_flags) + ["-c", s, "-o", o])

    def run(cmd):
        # cmd ends in "-o <target>": produce <target>.tmp.<pid>, then rename over the target (atomic on one filesystem)
        at = cmd.index("-o") + 1
        target = cmd[at]
        tmp = "%s.tmp.%d" % (target, os.getpid())
        cmd = cmd[:at] + [tmp] + cmd[at + 1:]
        try:
            _run(cmd)
            os.replace(tmp, target)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)

    def _run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n%s\n%s" % (" ".join(cmd), r.stderr[-8000:]))
        if verbose and r.stderr.strip():
            print(r.stderr[-4000:], file=sys.stderr)

    if jobs:
        with ThreadPoolExecutor(max_workers=len(jobs)) as ex:      # one hipcc per stale source
            list(ex.map(run, jobs))
    if jobs or force or _stale(lib, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs)
    return lib


def parse_user_arch(spec):
    """'32,64,64,1024' (filter counts of the reference trunks' layer shapes, then the fc width) or '32:8:4,64:5:2,512'
    (filters:size:stride per layer, then the fc width) -> (convs, fc)."""
    parts = str(spec).split(",")
    convs = []
    for i, p in enumerate(parts[:-1]):
        v = [int(x) for x in p.split(":")]
        if len(v) == 1:
            if i >= len(FAMILY):
                raise ValueError("more than three layers in %r" % (spec,))
            v = [v[0]] + list(FAMILY[i])
        if len(v) != 3:
            raise ValueError("layer %r: expected filters or filters:size:stride" % (p,))
        convs.append(tuple(v))
    return convs, int(parts[-1])


FAMILY = [(8, 4), (4, 2), (3, 1)]      # (kernel size, stride) of the reference trunks' layers (networks.py:145-149, :161-167)


def user_arch_library(convs, fc, variant=""):
    """In-tree path of the library compiled for a user architecture (convs: [(filters, size, stride), ...]); variant: the tag
    of a diagnostic build of it ("_rowdiv")."""
    convs = [tuple(int(v) for v in c) for c in convs]
    tag = "_".join(str(f) for f, _, _ in convs) + "_%d" % fc
    if any((k, s) != FAMILY[i] for i, (_, k, s) in enumerate(convs)):      # other layer shapes: they are part of the name
        tag += "_k" + "_".join("%dx%d" % (k, s) for _, k, s in convs)
    tag += variant
    return os.path.join(HERE, "libpaac_hip_user_%s.so" % tag), "_user_" + tag


def build_user_arch(convs, fc, verbose=False, variant="", variant_flags=()):
    """Compile libpaac_hip for a user architecture (include/paac_hip.h: PAAC_ARCH_USER; reference networks.py:117-120): two or
    three VALID conv layers (filters, size, stride) over the 84 x 84 x 4 input, then an fc layer.  The geometry is a
    compile-time template argument of every kernel, so a new architecture is a new build (about a minute of hipcc), cached
    in-tree by its shape (variant / variant_flags: a diagnostic build of it, under its own name).  The reference trunks' layer shapes -- conv 8x8 / 4, conv 4x4 / 2 [, conv 3x3 / 1] -- run on the MFMA
    data-gradient forms; any other kernel size / stride runs its forward and weight gradient on the same generic MFMA
    contraction (dmm.h) and its data gradient on a direct kernel.  Returns the library path."""
    convs = [tuple(int(v) for v in c) for c in convs]
    if len(convs) not in (2, 3) or any(len(c) != 3 for c in convs):
        raise NotImplementedError("user architectures have two or three conv layers (filters, size, stride); got %r" % (convs,))
    if any(f % 16 or f < 16 for f, _, _ in convs) or fc % 256 or fc < 256:
        raise NotImplementedError("filter counts must be multiples of 16 and the fc width a multiple of 256 (MFMA tiles); "
                                  "got %r, fc %d" % (convs, fc))
    if any(k < 1 or s < 1 for _, k, s in convs):
        raise ValueError("kernel sizes and strides must be positive; got %r" % (convs,))
    if (convs[0][1] * 4) % 16:
        raise NotImplementedError("the first layer's kernel size must be 4, 8, 12 or 16 (kernel width x 4 input channels is "
                                  "read in MFMA K groups of 16); got %d" % convs[0][1])
    size = 84
    for _, k, s in convs:
        if size < k:
            raise ValueError("layer shapes %r leave no output (VALID convolutions over 84 x 84)" % (convs,))
        size = (size - k) // s + 1
    lib, suffix = user_arch_library(convs, fc, variant)
    flags = list(variant_flags) + ["-DPAAC_USER_ARCH", "-DPAAC_USER_NCONV=%d" % len(convs), "-DPAAC_USER_C1=%d" % convs[0][0],
             "-DPAAC_USER_C2=%d" % convs[1][0], "-DPAAC_USER_C3=%d" % (convs[2][0] if len(convs) == 3 else 0),
             "-DPAAC_USER_H=%d" % fc]
    layers = convs + [(0, 3, 1)] * (3 - len(convs))
    flags += ["-DPAAC_USER_K%d=%d" % (i + 1, k) for i, (_, k, _) in enumerate(layers)]
    flags += ["-DPAAC_USER_S%d=%d" % (i + 1, st) for i, (_, _, st) in enumerate(layers)]
    try:
        return build(verbose=verbose, extra_flags=flags, lib_path=lib, obj_suffix=suffix)
    except RuntimeError as exc:
        raise RuntimeError("building the user architecture %s (fc %d) failed: %s" % (convs, fc, exc)) from exc


USER_GAME_SOURCES = ("games.hip",)      # the only source that reads PAAC_USER_GAME


def user_game_library(tag):
    """In-tree path of the library compiled for the user game `tag` (the specification module's file stem), and the suffix of
    its objects."""
    if not re.fullmatch(r"[A-Za-z0-9_]+", str(tag)):
        raise ValueError("device game tag %r (the specification module's file stem) must match [A-Za-z0-9_]+: it becomes part "
                         "of a library's file name" % (tag,))
    return os.path.join(HERE, "libpaac_hip_game_%s.so" % tag), "_game_" + tag


def _write_sidecar(sidecar, header, trait, digest):
    tmp = "%s.tmp.%d" % (sidecar, os.getpid())
    with open(tmp, "w") as f:
        f.write("%s\n%s\n%s\n" % (header, trait, digest))
    os.replace(tmp, sidecar)


def build_user_game(header, trait, tag, verbose=False):
    """Compile libpaac_hip with a user's device game in it (include/paac_hip.h: paac_user_game_info; the plugin contract is
    paac_amd/user_game.py's and csrc/game_dev.h's): `header` holds the trait struct `trait`, `tag` names the library.  Only
    games.hip reads the game, so only it is compiled again (a few seconds of hipcc); the other five objects are the stock
    build's, brought up to date first and held under the stock build's lock until the library is linked.  The header is among
    the dependencies: editing it rebuilds the library; a library newer than everything it was built from is
    returned as it is, whether or not the objects are still there.  Two different headers under one tag are refused -- the header's path, the
    trait and a digest of the header's text are kept in <library>.header; a recorded path that no longer exists or names the same file (the
    tree was moved, copied or is reached through a link) does not refuse, and the library stands if the text and the trait are the same.  Safe to call from several processes at once, like build().  Returns the library path."""
    lib, suffix = user_game_library(tag)
    header = os.path.abspath(header)
    if not os.path.isfile(header):
        raise FileNotFoundError("device game header %s not found" % header)
    if not re.fullmatch(r"[A-Za-z_][A-Za-z0-9_]*(::[A-Za-z_][A-Za-z0-9_]*)*", str(trait)):
        raise ValueError("device game trait %r is not the (qualified) name of a struct" % (trait,))
    sidecar = lib + ".header"
    flags = ["-DPAAC_USER_GAME", '-DPAAC_USER_GAME_HEADER="%s"' % header, "-DPAAC_USER_GAME_TRAIT=%s" % trait, "-I" + CSRC]
    with open(lib + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            digest = hashlib.sha256(open(header, "rb").read()).hexdigest()
            force = False
            if os.path.exists(sidecar):
                was = open(sidecar).read().split("\n")
                was_header, was_trait, was_digest = (was + ["", "", ""])[:3]
                if was_header != header and os.path.isfile(was_header) and not os.path.samefile(was_header, header):
                    raise ValueError("device game tag %r is taken: %s was built from %s, not from %s -- two games need two file "
                                     "stems (or remove that library)" % (tag, os.path.basename(lib), was_header, header))
                # the same path -- or the recorded header is gone: a tree that was moved or copied.  The same text and trait:
                # the same game, and its library stands if it is newer than everything it was built from, objects kept or not
                same = was_trait == trait and was_digest == digest
                if same and library_is_current(lib, [header]):
                    if was_header != header:
                        _write_sidecar(sidecar, header, trait, digest)
                    return lib
                force = not same
            with open(LIB + ".lock", "w") as stock:          # lock order: the game's, then the stock build's
                fcntl.flock(stock, fcntl.LOCK_EX)
                try:
                    _build_locked(False, verbose, (), LIB, "")
                    _build_locked(force, verbose, flags, lib, suffix, extra_deps=[header], only=USER_GAME_SOURCES)
                finally:
                    fcntl.flock(stock, fcntl.LOCK_UN)
            _write_sidecar(sidecar, header, trait, digest)
            return lib
        except RuntimeError as exc:
            raise RuntimeError("building the device game %s (%s in %s) failed: %s" % (tag, trait, header, exc)) from exc
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


ROWDIV_FLAGS = ["-DPAAC_WGRAD_ROW_WALK=0"]


def rowdiv_library(spec=None):
    """In-tree path of the build whose weight gradients decompose their patch rows by division per load (csrc/dmm.h:
    PAAC_WGRAD_ROW_WALK=0) instead of walking them: the stock library, or the one of user architecture `spec`."""
    if spec is None:
        return os.path.join(HERE, "libpaac_hip_rowdiv.so")
    return user_arch_library(*parse_user_arch(spec), variant="_rowdiv")[0]


def build_rowdiv(spec=None, verbose=False):
    if spec is None:
        return build(verbose=verbose, extra_flags=ROWDIV_FLAGS, lib_path=rowdiv_library(), obj_suffix="_rowdiv")
    return build_user_arch(*parse_user_arch(spec), verbose=verbose, variant="_rowdiv", variant_flags=ROWDIV_FLAGS)


if __name__ == "__main__":
    if "--user-arch" in sys.argv:        # e.g. --user-arch 32,64,64,1024 (filter counts, then the fc width), or
        spec = sys.argv[sys.argv.index("--user-arch") + 1]          # 32:8:4,64:5:2,64:3:1,512 (filters:size:stride per layer)
        print(build_user_arch(*parse_user_arch(spec), verbose=True))
    elif "--stamps" in sys.argv or "--ksplit" in sys.argv or "--rowdiv" in sys.argv:
        # --stamps: cycle stamps inside the kernels (tools/probe_*stamps.py); --ksplit: the conv tower's small regions on the K
        # split over wave pairs instead of GEMM / helper wave roles (csrc/tower.h: PAAC_T_ROLES), for A/B runs; --rowdiv: the
        # weight gradients' patch rows decomposed by division per load instead of walked (csrc/dmm.h: PAAC_WGRAD_ROW_WALK),
        # for A/B runs and tests/test_wgrad_row_walk_gpu.py.  They combine.
        variants = [("--stamps", "_stamps", "-DPAAC_DMM_STAMPS"), ("--ksplit", "_ksplit", "-DPAAC_T_ROLES=0"),
                    ("--rowdiv", "_rowdiv", "-DPAAC_WGRAD_ROW_WALK=0")]
        tag = "".join(t for a, t, _ in variants if a in sys.argv)
        flags = [f for a, _, f in variants if a in sys.argv]
        print(build(extra_flags=flags, lib_path=os.path.join(HERE, "libpaac_hip%s.so" % tag), obj_suffix=tag))
    else:
        print(build(force="--force" in sys.argv))
