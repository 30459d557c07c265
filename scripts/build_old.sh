#!/bin/bash
# A/B baseline: prego_amd/lib_ab/libold.so = the library of git HEAD (sources of HEAD for the files given, the tree's objects for the rest).
#   bash scripts/build_old.sh gru_recurrence.hip [more files of prego_amd/csrc ...]      (run next to `python -m prego_amd.build`)
#   DEBUG=1 bash scripts/build_old.sh ...     prego_amd/lib_ab/libold_debug.so: the same with the debug library's objects (host files
#                                             compiled with -DPREGO_DEBUG_ABI), for probes that call prego_debug_* entries of both
# The object list is HEAD's source list, so a file that the tree no longer has must be among the files given.
set -e
cd "$(dirname "$0")/.."
rm -rf prego_amd/lib_ab/_oldsrc && mkdir -p prego_amd/lib_ab/_oldsrc prego_amd/lib_ab
git archive HEAD prego_amd/csrc include | tar -x -C prego_amd/lib_ab/_oldsrc
dbg=""; out=libold.so
if [ -n "$DEBUG" ]; then dbg="-DPREGO_DEBUG_ABI"; out=libold_debug.so; fi
obj_of() {     # the object name prego_amd/build.py gives a source
  case $1 in *.cpp) if [ -n "$DEBUG" ]; then echo "$(echo $1 | tr . _)_dbg.o"; else echo "$(echo $1 | tr . _).o"; fi;; *) echo "$(echo $1 | tr . _).o";; esac
}
for f in "$@"; do
  x=""; case $f in *.cpp) x="-x hip $dbg";; esac
  (cd prego_amd/lib_ab/_oldsrc && /opt/rocm/bin/hipcc -O3 -fPIC -std=c++17 --offload-arch=gfx950 -Wno-unused-result -Wno-inline-asm $x -c prego_amd/csrc/$f -o $(obj_of $f)) &
done
wait
objs=""
for s in $(git ls-tree --name-only HEAD prego_amd/csrc/ | grep -E '\.(hip|cpp)$'); do
  b=$(basename $s)
  if [ -z "$DEBUG" ] && [ "$b" = debug_hog.hip ]; then continue; fi       # build.py: DEBUG_ONLY_SOURCES
  o=$(obj_of $b)
  if [ -f prego_amd/lib_ab/_oldsrc/$o ]; then objs="$objs prego_amd/lib_ab/_oldsrc/$o"; else objs="$objs prego_amd/lib/$o"; fi
done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o prego_amd/lib_ab/$out $objs
echo prego_amd/lib_ab/$out
