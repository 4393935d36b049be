# Builds the C-ABI HIP library (gfx950 only) and the oracle-side helpers.
HIPCC ?= /opt/rocm/bin/hipcc
ARCH  ?= gfx950
SRC   := $(wildcard fedmlp_amd/csrc/*.hip)
HDR   := $(wildcard fedmlp_amd/csrc/*.h) include/fedmlp_hip.h include/fedmlp_hip_debug.h include/fedmlp_hip_rofl.h \
         include/fedmlp_hip_drift.h include/fedmlp_hip_server.h
# every fedmlp_amd/csrc/*.hip is a translation unit of the library (drift.hip, the client-drift correction, and server_opt.hip,
# the server optimizers, among them)
OBJ   := $(patsubst fedmlp_amd/csrc/%.hip,build/%.o,$(SRC))
LIB   := fedmlp_amd/libfedmlp_hip.so

all: $(LIB)

build/%.o: fedmlp_amd/csrc/%.hip $(HDR)
	@mkdir -p build
	$(HIPCC) --offload-arch=$(ARCH) -O3 -fPIC -std=c++17 -Wall -Wno-unused-function -c $< -o $@

$(LIB): $(OBJ)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJ)

clean:
	rm -rf build $(LIB)

# measurement-only artefacts (tuning / probe builds, assembly dumps): nothing of the product depends on them
clean-scratch:
	rm -rf scratch tune build/*.s __pycache__ .pytest_cache

.PHONY: all clean clean-scratch
