# Dev helper: a -DFER_PROBE build of the library next to the product one (h264-fer_amd/libferhip_probe.so).
# EVERY object is rebuilt (-B), in a directory of its own: the kernels take FerDev by value, objects built against
# different fer_dev.h layouts fault.  The file list is the Makefile's.
set -e
make -B -j8 -C "$(dirname "$0")/../h264-fer_amd/csrc" EXTRA=-DFER_PROBE OBJDIR=build/probe OUT=../libferhip_probe.so
ls -la "$(dirname "$0")/../h264-fer_amd/libferhip_probe.so"
