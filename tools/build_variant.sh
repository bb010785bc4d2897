# Build a variant of libtfusion_hip.so with extra defines into tools/_build/NAME/ (for A/B runs
# through TFUSION_HIP_LIB, tools/gpu_ab_lib.sh), by the library's own Makefile.
#   bash tools/build_variant.sh NAME -DX=1 ...
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
NAME=$1; shift
O=$R/tools/_build/$NAME
mkdir -p $O
make -s -j8 -C $R/topfusion_amd/csrc OBJDIR=$O OUT=$O/libtfusion_hip.so DEFS="$*"
rm -f $O/*.o
echo "built $O/libtfusion_hip.so"
