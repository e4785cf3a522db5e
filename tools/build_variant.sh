#!/bin/bash
# A second build of libicelk.so from the sources as they are NOW (plus -D flags), for A/B runs on one GPU box:
#   tools/build_variant.sh <name> [extra hipcc flags]   ->  variants/libicelk_<name>.so   (select with ICELK_LIBRARY=...)
# Sources and flags are build.py's: there is one list.
set -e
NAME=$1; shift
cd "$(dirname "$0")/.."
mkdir -p variants
python3 -c "
import sys
from iceberg_tracking_code_amd import build as b
b.build(force=True, lib='variants/libicelk_%s.so' % sys.argv[1], obj_dir='variants/obj_' + sys.argv[1], extra_flags=sys.argv[2:])
" "$NAME" "$@"
rm -rf variants/obj_$NAME
ls -la variants/libicelk_$NAME.so
