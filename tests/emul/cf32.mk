# TEST-ONLY host build of the cf32 code of fft_core.h (8-byte raw layout, the float unpack, cf32 against cs16 through
# the emulated transform): cf32_emul.cpp -> librpf_emul_cf32.so, loaded by tests/test_cf32.py.  A makefile of its own
# (make -f cf32.mk) beside the emulator's, as formats.mk.  The rows come from k1_sizes.h, which includes the HIP runtime
# header: ROCm's clang compiles the file as HIP for the host alone (no device pass, no GPU code in the library, which is linked without the HIP runtime).
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_cf32.so: cf32_emul.cpp $(CSRC)/fft_core.h $(CSRC)/k1_sizes.h $(CSRC)/rpf_device_common.h
	$(CXX) -x hip --offload-host-only --rocm-path=/opt/rocm -O1 -std=c++17 -fPIC -ffp-contract=off -c -o cf32_emul.host.o cf32_emul.cpp
	$(CXX) -shared -o $@ cf32_emul.host.o
	rm -f cf32_emul.host.o
clean:
	rm -f librpf_emul_cf32.so
.PHONY: clean
