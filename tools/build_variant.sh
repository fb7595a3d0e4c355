#!/bin/bash
# A/B aid: tools/bin/ab_<name>.so = the product library with extra flags on chosen translation units
#   bash tools/build_variant.sh <name> "-DQA_EXP_..." ["w4a16_xk w4a16_xw"] [tools]
# (third argument: the units to recompile with the flags, default the exchange kernels; the unit list and every unit's own extra flags --
# the kernarg preload of the lean / xm / xw / xk units -- are quick_amd.build's SOURCES and EXTRA_CFLAGS)
name=$1; defs=$2; units=${3:-"w4a16_xk w4a16_xw"}
root=$(cd "$(dirname "$0")/.." && pwd)
cd "$root" || exit 1
base=$root/quick_amd/lib/obj
if [ "$4" = tools ]; then base=$root/tools/bin/obj_tools; defs="$defs -DQUICK_AMD_TOOLS"; python -m quick_amd.build --tools > /dev/null || exit 1; else python -m quick_amd.build > /dev/null || exit 1; fi
o=$root/tools/bin/obj_ab_$name; mkdir -p $o
hipcc=$(python -c "from quick_amd import build; print(build._hipcc())") || exit 1
cflags=$(python -c "from quick_amd import build; print(' '.join(build.CFLAGS))")
ldflags=$(python -c "from quick_amd import build; print(' '.join(build.LDFLAGS))")
objs=""
while read -r f extra; do      # one line per unit: its name without .hip, then its own extra flags
  if echo " $units " | grep -q " $f "; then
    $hipcc $cflags $extra $defs -c -o $o/$f.o $root/quick_amd/csrc/$f.hip &
    objs="$objs $o/$f.o"
  else
    objs="$objs $base/$f.o"
  fi
done < <(python -c "
from quick_amd import build
for s in build.SOURCES: print(s[:-4], *build.EXTRA_CFLAGS.get(s, []))")
wait
$hipcc $ldflags -o $root/tools/bin/ab_$name.so $objs || exit 1
ls -la $root/tools/bin/ab_$name.so
