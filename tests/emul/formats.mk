# TEST-ONLY host build of the sample-format code of fft_core.h alone (signed unpacks, the 16-bit raw layout):
# formats_emul.cpp -> librpf_emul_formats.so, loaded by tests/test_sample_formats.py.  A makefile of its own
# (make -f formats.mk) beside the emulator's; ROCm's clang because fft_core.h uses clang's ext_vector_type.
CXX := /opt/rocm/lib/llvm/bin/clang++
librpf_emul_formats.so: formats_emul.cpp ../../rtl-power-fftw_amd/csrc/fft_core.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -ffp-contract=off -o $@ formats_emul.cpp
clean:
	rm -f librpf_emul_formats.so
.PHONY: clean
