# The statements of the MCMC densification strategy (gaussiansplat_amd/csrc/gs_mcmc.h) as HOST code:
#     make -C tests -f mcmc.mk mcmc-host        builds tests/_build/mcmc_host, the program tests/test_mcmc_host.py feeds its cases
#     make -C tests -f mcmc.mk sanitize-mcmc    builds it under AddressSanitizer + UndefinedBehaviorSanitizer and runs it without arguments
#                                               (its built-in scene: NaN and infinite opacities, the edge draws, counts beyond the table)
# tests/mcmc_host.cpp is a stand-alone program with its own main.  No python, no LD_PRELOAD, no device.  Every sanitizer option stands behind
# -Xarch_host: the host side only, never a device code object.  A file of its own beside tests/Makefile and tests/exposure.mk, which stay as
# they are; the three share the build folder.
HIPCC ?= /opt/rocm/bin/hipcc
OUT := _build
CSRC := ../gaussiansplat_amd/csrc
DEPS := mcmc_host.cpp $(CSRC)/gs_mcmc.h $(CSRC)/gs_pergaussian.h $(CSRC)/gs_detmath.h

.PHONY: mcmc-host sanitize-mcmc clean
mcmc-host: $(OUT)/mcmc_host

sanitize-mcmc: $(OUT)/mcmc_host_asan
	ASAN_OPTIONS=detect_leaks=1:abort_on_error=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 ./$(OUT)/mcmc_host_asan

$(OUT)/mcmc_host: $(DEPS)
	@mkdir -p $(OUT)
	$(HIPCC) -O2 -std=c++17 -x hip --cuda-host-only -Wall -ffp-contract=off -I $(CSRC) -I ../include mcmc_host.cpp -o $@

$(OUT)/mcmc_host_asan: $(DEPS)
	@mkdir -p $(OUT)
	$(HIPCC) -O1 -g -std=c++17 -x hip --cuda-host-only -Wall -ffp-contract=off -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined \
	  -Xarch_host -fno-sanitize-recover=undefined -fno-omit-frame-pointer \
	  -I $(CSRC) -I ../include mcmc_host.cpp -o $@

clean:
	rm -rf $(OUT)
