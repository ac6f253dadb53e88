# Dev helper: a variant build of the library for A/B timing on one box: tools/build_variant.sh NAME "-DRES_WAVES=5 ..."
# -> h264-fer_amd/var/libferhip_NAME.so (every object rebuilt with the flags, the file list is the Makefile's; swap it in
#    with cp h264-fer_amd/var/libferhip_NAME.so h264-fer_amd/libferhip.so on the GPU box's scratch copy)
set -e
name=$1; flags=$2
make -B -j8 -C "$(dirname "$0")/../h264-fer_amd/csrc" EXTRA="$flags" OBJDIR=build/var_$name OUT=../var/libferhip_$name.so
ls -la "$(dirname "$0")/../h264-fer_amd/var/libferhip_$name.so"
