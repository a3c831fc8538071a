# TEST-ONLY host build of the series partition (rtl-power-fftw_amd/csrc/series_partition.h): the arithmetic table, the
# complete / cut rule, the slots and the fix-up's closed forms, and a walk of the partition the way the kernel and the
# fix-up kernel walk it: series_emul.cpp -> librpf_emul_series.so, loaded by tests/test_series.py.  A makefile of its own
# (make -f series.mk) beside the emulator's, as formats.mk and stats.mk.
CXX := /opt/rocm/lib/llvm/bin/clang++
CSRC := ../../rtl-power-fftw_amd/csrc
librpf_emul_series.so: series_emul.cpp $(CSRC)/series_partition.h $(CSRC)/hop_partition.h
	$(CXX) -O1 -std=c++17 -fPIC -shared -ffp-contract=off -o $@ series_emul.cpp
clean:
	rm -f librpf_emul_series.so
.PHONY: clean
