#!/usr/bin/env bash
# Is the gfx950 device code of this tree the same as another tree's?  No GPU needed.
#   usage: tools/device_code_diff.sh <other-csrc-dir> [hipcc flags]
# <other-csrc-dir>: noisereduce_amd/csrc of another checkout (git worktree add, git archive | tar -x: the units include ../../include).
# Compiles every .hip unit of both csrc directories (DCD_UNITS="api.hip ..." restricts them) with the flags of
# __graft_entry__.build() + the given ones + --cuda-device-only --no-gpu-bundle-output -c, at most DCD_JOBS (default and
# ceiling 16) compilers at a time, disassembles each object (llvm-objdump -d --no-show-raw-insn; addresses and the
# file-name line stripped) and compares the text function symbol by function symbol.  Prints one line per unit -- the
# number of function symbols on either side and how many differ -- and the names of those that differ or exist on one
# side only; exits 1 if there is any.  DCD_KEEP=<dir> keeps objects and listings there (default: a scratch directory).
set -euo pipefail
[ $# -ge 1 ] || { sed -n '2,4p' "$0" >&2; exit 2; }
root="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
other="$(cd "$1" && pwd)"; shift
mine="$root/noisereduce_amd/csrc"
jobs="${DCD_JOBS:-16}"; [ "$jobs" -le 16 ] || jobs=16
rocm="${ROCM_PATH:-/opt/rocm}"
if [ -n "${DCD_KEEP:-}" ]; then work="$(realpath -m "$DCD_KEEP")"; else work="$(mktemp -d)"; trap 'rm -rf "$work"' EXIT; fi
mkdir -p "$work/this" "$work/other"
units="$(printf '%s\n' ${DCD_UNITS:-$(cd "$mine" && ls *.hip; cd "$other" && ls *.hip)} | sort -u)"

list() {   # <side> <csrc dir> <unit> [flags]: compile, disassemble, strip what depends on where the code lies
  local side=$1 dir=$2 u=$3; shift 3
  local o="$work/$side/${u%.hip}"
  [ -e "$dir/$u" ] || { : > "$o.s"; return 0; }   # (a unit only the other tree has: every symbol of it is reported)
  (cd "$dir" && "$rocm/bin/hipcc" --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden \
     -Xclang -target-feature -Xclang -packed-fp32-ops "$@" --cuda-device-only --no-gpu-bundle-output -c "$u" -o "$o.o") 2> "$o.log"
  "$rocm/llvm/bin/llvm-objdump" -d --no-show-raw-insn "$o.o" \
    | sed -e '/file format/d' -e 's/^[0-9a-f]\{8,\} </</' -e 's/[ \t]*\/\/ [0-9A-Fa-f]\{8,\}:.*$//' > "$o.s"
}
pids=()
for u in $units; do
  for side in this other; do
    while [ "$(jobs -rp | wc -l)" -ge "$jobs" ]; do wait -n || true; done
    if [ $side = this ]; then list this "$mine" "$u" "$@" & else list other "$other" "$u" "$@" & fi
    pids+=($!)
  done
done
failed=0
for p in "${pids[@]}"; do wait "$p" || failed=1; done   # (every compiler has ended before the scratch directory goes)
if [ $failed = 1 ]; then
  echo "a compile failed; the logs that name an error:" >&2
  grep -l "error" "$work"/*/*.log | while read -r f; do echo "-- $f" >&2; grep -m 5 -A 2 "error" "$f" >&2; done
  exit 2
fi

python3 - "$work" $units <<'PY'
import re, sys
work, units = sys.argv[1], sys.argv[2:]
def functions(path):
    out, name = {}, None
    for ln in open(path, errors="replace"):
        m = re.match(r"<(.+)>:\s*$", ln)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None and ln.strip() and not ln.startswith("Disassembly of section"):
            out[name].append(ln.rstrip())
    return out
bad = 0
for u in units:
    a, b = (functions("%s/%s/%s.s" % (work, side, u[:-4])) for side in ("this", "other"))
    only = sorted(set(a) ^ set(b))
    diff = sorted(n for n in set(a) & set(b) if a[n] != b[n])
    print("%-18s function symbols: %d vs %d, %s, differing: %d" % (u, len(a), len(b), "same set" if not only else "%d on one side only" % len(only), len(diff)))
    for n in only:
        print("    only in %s: %s" % ("this tree" if n in a else "the other tree", n))
    for n in diff:
        print("    differs: %s" % n)
    bad += len(only) + len(diff)
print("total differing or one-sided: %d" % bad)
sys.exit(1 if bad else 0)
PY
