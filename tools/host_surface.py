"""Host-only surface of two builds of libralenet.so, compared call by call (no GPU): every configuration entry point over a grid
of configurations, return values and ral_last_error() after each failure.

    python tools/host_surface.py OLD/libralenet.so NEW/libralenet.so

prints the number of cases, then every case whose records differ (first differing call of each), grouped by message pair."""
import collections
import ctypes as C
import itertools
import sys
import zlib

VARIANTS = [-1, 0, 1, 2, 3, 4, 5, 6]
LS = [0, 16, 32, 48, 64, 256, 320, 500, 512, 520, 1024, 1040, 2048, 2064]


class Cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("variant", "leads", "L", "max_batch", "train")]


def load(path):
    L = C.CDLL(path)
    L.ral_last_error.restype = C.c_char_p
    for n in ("ral_param_floats", "ral_state_floats", "ral_bn_sums_doubles", "ral_workspace_bytes"):
        getattr(L, n).restype = C.c_int64
    L.ral_pe_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]
    return L


def record(L, cfg):
    """[(call, return value, error text or results)] of one configuration"""
    out, p = [], C.byref(cfg)
    def note(call, rc, *res):
        out.append((call, rc, L.ral_last_error().decode() if rc != 0 and not res else res))
    count = L.ral_layout_count(p)
    out.append(("count", count, L.ral_last_error().decode() if count < 0 else ""))
    name, kind, off, nd, shp = C.create_string_buffer(256), C.c_int32(), C.c_int64(), C.c_int32(), (C.c_int64 * 4)()
    for idx, cap in [(i, 256) for i in range(-1, max(count, 0) + 1)] + [(0, 1)]:
        rc = L.ral_layout_entry(p, idx, name, cap, C.byref(kind), C.byref(off), C.byref(nd), shp)
        out.append((f"entry {idx} cap {cap}", rc, (name.value, kind.value, off.value, nd.value, tuple(shp)) if rc == 0 else L.ral_last_error().decode()))
    for n in ("ral_param_floats", "ral_state_floats", "ral_bn_sums_doubles", "ral_workspace_bytes"):
        rc = getattr(L, n)(p)
        out.append((n, rc, L.ral_last_error().decode() if rc < 0 else ""))
    for level in range(-1, 6):
        buf = (C.c_float * (2064 * 128))()
        rc = L.ral_pe_table(p, level, buf, len(buf))
        out.append((f"pe_table {level}", rc, "table crc %08x" % zlib.crc32(bytes(buf)) if rc == 0 else L.ral_last_error().decode()))
    return out


def main(old_path, new_path):
    old, new = load(old_path), load(new_path)
    cases = differing = 0
    groups = collections.Counter()
    for v, leads, Lw, mb, tr in itertools.product(VARIANTS, [1, 2, 3], LS, [0, 1, 4, 2048], [0, 1]):
        cfg = Cfg(v, leads, Lw, mb, tr)
        a, b = record(old, cfg), record(new, cfg)
        cases += 1
        diffs = [(x, y) for x, y in zip(a, b) if x != y]
        if len(a) != len(b) or diffs:
            differing += 1
            for x, y in diffs:
                call = x[0].split()[0] + (" (name_cap 1)" if x[0].endswith("cap 1") else " (bad index)" if x[0].startswith("entry") else "")
                groups[(v, call, x[1], str(x[2])[:70].split(" crc")[0], y[1], str(y[2])[:70].split(" crc")[0])] += 1
    print(f"{cases} configurations, {differing} with a differing record")
    for (v, call, r0, t0, r1, t1), n in sorted(groups.items()):
        print(f"  variant {v} {call}: {n} calls: {r0} '{t0}' -> {r1} '{t1}'")


if __name__ == "__main__":
    main(*sys.argv[1:3])
