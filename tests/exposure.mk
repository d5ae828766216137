# Host sanitizers on the statements of the per-view exposure stage (gaussiansplat_amd/csrc/gs_exposure.h):
#     make -C tests -f exposure.mk sanitize-exposure
# builds tests/exposure_host.cpp, a stand-alone program with its own main, as HOST code under AddressSanitizer + UndefinedBehaviorSanitizer
# and runs it without arguments (its built-in scene: odd sizes, weights of 0 and 1, identity rows, a -0 sample).  No python, no LD_PRELOAD,
# no device.  Every sanitizer option stands behind -Xarch_host: the host side only, never a device code object.  A file of its own beside
# tests/Makefile (sanitize-camera-grad), which stays as it is; the two share the build folder.
HIPCC ?= /opt/rocm/bin/hipcc
OUT := _build

.PHONY: sanitize-exposure clean
sanitize-exposure: $(OUT)/exposure_host_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 ./$(OUT)/exposure_host_asan

$(OUT)/exposure_host_asan: exposure_host.cpp ../gaussiansplat_amd/csrc/gs_exposure.h
	@mkdir -p $(OUT)
	$(HIPCC) -O1 -g -std=c++17 -x hip --cuda-host-only -Wall -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
	  -I ../gaussiansplat_amd/csrc -I ../include exposure_host.cpp -o $@

clean:
	rm -rf $(OUT)
