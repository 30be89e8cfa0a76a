"""Decode the reference's MD5 test vectors through front-end + oracle (container only: reads
/root/reference/tests/dav1d-test-data). Prints one line per vector: ok / MISMATCH / error. The
[name, file, md5] triples run with default settings; the explicit test() entries run with the
settings their arguments name (--oppoint, --alllayers, --decodeframetype, --filmgrain).

    python tools/scan_vectors.py [substring ...]
"""
import os
import re
import sys
import time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DATA = "/root/reference/tests/dav1d-test-data"


def vectors():
    out = []
    for d, _, files in os.walk(DATA):
        if "meson.build" not in files:
            continue
        txt = open(os.path.join(d, "meson.build")).read()
        for name, f, md5 in re.findall(r"\['([^']+)',\s*files\('([^']+)'\),\s*'([0-9a-f]{32})'\]", txt):
            out.append((name, os.path.join(d, f), md5))
    return sorted(out)


def explicit_tests():
    """The explicit test(...) entries of the meson files whose input exists:
    [(name, path, md5, args)], args = {oppoint, alllayers, decodeframetype, filmgrain} with the
    CLI's defaults (tools/dav1d_cli_parse.rs) for the options an entry leaves out."""
    out = []
    for d, _, files in sorted(os.walk(DATA)):
        if "meson.build" not in files:
            continue
        txt = open(os.path.join(d, "meson.build")).read()
        for name, body in re.findall(r"^\s*test\('([^']+)',\s*dav1d,(.*?)\]\s*\)", txt, re.S | re.M):
            f = re.search(r"files\('([^']+)'\)", body)
            md5 = re.search(r"'--verify',\s*'([0-9a-f]{32})'", body)
            if not f or not md5 or not os.path.exists(os.path.join(d, f.group(1))):
                continue
            opts = dict(re.findall(r"'--([a-z]+)',\s*'([^']*)'", body))
            unknown = set(opts) - {"verify", "oppoint", "alllayers", "decodeframetype", "filmgrain"}
            assert not unknown and "--limit" not in body, (name, unknown)
            args = {"oppoint": int(opts.get("oppoint", 0)), "alllayers": int(opts.get("alllayers", 1)),
                    "decodeframetype": opts.get("decodeframetype", "all"), "filmgrain": int(opts.get("filmgrain", 0))}
            out.append((name, os.path.join(d, f.group(1)), md5.group(1), args))
    return out


def entry_name(name, args):
    """A unique name for an explicit entry: the meson name plus the arguments that are not defaults."""
    tags = [f"op{args['oppoint']}"] if (args["oppoint"] or not args["alllayers"]) else []
    tags += [] if args["alllayers"] else ["top"]
    tags += [] if args["decodeframetype"] == "all" else [args["decodeframetype"]]
    tags += ["fg"] if args["filmgrain"] else []
    return "-".join([name] + tags)


def decode_with(data, args, threads=1):
    """(md5, pictures) of a stream through front-end + oracle with an explicit entry's settings."""
    from tests.settings_lib import decode_settings
    r = decode_settings(data, threads=threads, apply_grain=bool(args["filmgrain"]), operating_point=args["oppoint"],
                        all_layers=bool(args["alllayers"]), decode_frame_type=args["decodeframetype"])
    return r.md5, len(r.sizes)


def run(v):
    name, path, md5 = v[:3]
    from tests.stream_lib import decode_stream
    t = time.time()
    try:
        if len(v) > 3:
            name = entry_name(name, v[3])
            got, n = decode_with(open(path, "rb").read(), v[3])
        else:
            got, n = decode_stream(open(path, "rb").read())
    except Exception as e:  # noqa: BLE001 - report and continue
        return f"error    {name} {type(e).__name__}: {str(e)[:120]}"
    tag = "ok      " if got == md5 else "MISMATCH"
    return f"{tag} {name} frames={n} {time.time() - t:.1f}s {os.path.getsize(path)}B"


if __name__ == "__main__":
    vs = [v for v in vectors() + explicit_tests()
          if not sys.argv[1:] or any(s in v[0] or s in v[1] for s in sys.argv[1:])]
    with ProcessPoolExecutor(int(os.environ.get("JOBS", "6"))) as ex:
        for line in ex.map(run, vs):
            print(line, flush=True)
