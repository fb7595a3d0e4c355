#!/bin/bash
# A/B aid: tools/bin/ab_<name>.so = the product library with extra flags on chosen translation units
#   bash tools/build_variant.sh <name> "<flags>" ["w4a16_xk w4a16_xw"] [tools] [patch]
# (third argument: the units to recompile with the flags, default the exchange kernels; the unit list and every unit's own extra flags --
# the kernarg preload of the lean / xm / xw / xk units -- are quick_amd.build's SOURCES and EXTRA_CFLAGS)
# Fifth argument: an experiment parked under tools/patches/ (tools/patches/README.md has the flags and units of each).  The patch is applied to
# a COPY of the sources, tools/bin/src_ab_<name>/ (quick_amd/csrc, include and the two loop generators, laid out as in the tree), and the
# chosen units are compiled from there: the working tree, the product library and its source stamp stay as they are.  A patch that changes
# tools/gen_xm_loop.py has the copy's generator rewrite the copy's w4a16_xm_loop.inc, under whatever XM_* switches the caller's environment sets.
name=$1; defs=$2; units=${3:-"w4a16_xk w4a16_xw"}; patch=$5
root=$(cd "$(dirname "$0")/.." && pwd)
if [ -n "$patch" ]; then patch=$(cd "$(dirname "$patch")" && pwd)/$(basename "$patch"); [ -f "$patch" ] || { echo "no such patch: $5" >&2; exit 1; }; fi
cd "$root" || exit 1
base=$root/quick_amd/lib/obj
if [ "$4" = tools ]; then base=$root/tools/bin/obj_tools; defs="$defs -DQUICK_AMD_TOOLS"; python -m quick_amd.build --tools > /dev/null || exit 1; else python -m quick_amd.build > /dev/null || exit 1; fi
src=$root/quick_amd/csrc
if [ -n "$patch" ]; then
  copy=$root/tools/bin/src_ab_$name
  rm -rf "$copy"; mkdir -p "$copy/quick_amd" "$copy/tools" || exit 1
  cp -r "$root/quick_amd/csrc" "$copy/quick_amd/" && cp -r "$root/include" "$copy/" && cp "$root/tools/gen_xm_loop.py" "$root/tools/gen_xw_loop.py" "$copy/tools/" || exit 1
  # (the ceiling keeps git from finding the repository above the copy: it applies the patch to the files where it stands, as outside a repository)
  (cd "$copy" && GIT_CEILING_DIRECTORIES=$root/tools/bin git apply "$patch") || exit 1
  if ! cmp -s "$copy/tools/gen_xm_loop.py" "$root/tools/gen_xm_loop.py"; then python "$copy/tools/gen_xm_loop.py" > /dev/null || exit 1; fi
  src=$copy/quick_amd/csrc
fi
o=$root/tools/bin/obj_ab_$name; mkdir -p $o
hipcc=$(python -c "from quick_amd import build; print(build._hipcc())") || exit 1
cflags=$(python -c "from quick_amd import build; print(' '.join(build.CFLAGS))")
ldflags=$(python -c "from quick_amd import build; print(' '.join(build.LDFLAGS))")
objs=""; pids=""
while read -r f extra; do      # one line per unit: its name without .hip, then its own extra flags
  if echo " $units " | grep -q " $f "; then
    $hipcc $cflags $extra $defs -c -o $o/$f.o $src/$f.hip &
    pids="$pids $!"
    objs="$objs $o/$f.o"
  else
    objs="$objs $base/$f.o"
  fi
done < <(python -c "
from quick_amd import build
for s in build.SOURCES: print(s[:-4], *build.EXTRA_CFLAGS.get(s, []))")
for p in $pids; do wait $p || exit 1; done
$hipcc $ldflags -o $root/tools/bin/ab_$name.so $objs || exit 1
ls -la $root/tools/bin/ab_$name.so
