# The harness of the ggml-backend glue for multi-sequence graphs over long caches
# (tests/adapter/multiseq_longctx_test.cpp, host code, g++): built by __graft_entry__.build()
# into tests/adapter/bin/ beside glue_test, with the same flags (-Werror against the restated
# ggml-backend-impl.h subset).
#   make -C tests/adapter -f multiseq_longctx.mk
ROOT := $(abspath $(dir $(lastword $(MAKEFILE_LIST)))/../..)
BIN ?= $(ROOT)/tests/adapter/bin
LIB := $(ROOT)/ggml-neon-opt_amd/lib
CXXFLAGS := -std=c++17 -O1 -g -Wall -Wextra -Werror -DGGML_BACKEND_DL \
            -I$(ROOT)/include -I$(ROOT)/ggml-neon-opt_amd/adapter -I$(ROOT)/tests/adapter/ggml -I$(ROOT)/tests/adapter
SRCS := $(ROOT)/ggml-neon-opt_amd/adapter/ggml-mi355x.cpp $(ROOT)/tests/adapter/ggml_stub.cpp $(ROOT)/tests/adapter/multiseq_longctx_test.cpp
DEPS := $(SRCS) $(ROOT)/ggml-neon-opt_amd/adapter/ggml-mi355x.h $(ROOT)/ggml-neon-opt_amd/adapter/mi355x_ggml_mirror.hpp \
        $(wildcard $(ROOT)/tests/adapter/ggml/*.h) $(ROOT)/tests/adapter/ggml_stub.h $(ROOT)/include/ggml_mi355x.h

all: $(BIN)/multiseq_longctx_test

$(BIN)/multiseq_longctx_test: $(DEPS) $(LIB)/libggml_mi355x.so
	@mkdir -p $(BIN)
	g++ $(CXXFLAGS) $(SRCS) -o $@ -L$(LIB) -lggml_mi355x -Wl,-rpath,'$$ORIGIN/../../../ggml-neon-opt_amd/lib' -Wl,-rpath,$(LIB)

.PHONY: all
