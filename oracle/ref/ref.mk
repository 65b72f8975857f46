# oracle/ref/ref.mk — run from oracle/ by `make ref`: compiles the reference model's own sources, in place from the
# checkout at SHUD_REF, with our driver / dispatcher and the vector-container stand-ins of ref/nvector/, into _ref/.
# Flags are the reference Makefile's own (-O3 -std=c++14; x86-64 g++ emits no FMA there).  The three units that
# need CVODE itself (cvode_config.cpp, print.cpp, shud.cpp) and main.cpp are left out.  Nothing under _ref/ is
# committed; the programs and the library there need no object file at run time.
CXX ?= g++
REFFLAGS = -O3 -std=c++14 -w
SRC = $(SHUD_REF)/src
INC = -Iref -I$(SRC)/Model -I$(SRC)/ModelData -I$(SRC)/classes -I$(SRC)/Equations
UNITS := $(filter-out $(SRC)/Equations/cvode_config.cpp $(SRC)/Equations/print.cpp $(SRC)/Model/shud.cpp, \
           $(wildcard $(SRC)/classes/*.cpp $(SRC)/ModelData/*.cpp $(SRC)/Model/*.cpp $(SRC)/Equations/*.cpp))
NAMES := $(basename $(notdir $(UNITS)))
vpath %.cpp $(SRC)/classes $(SRC)/ModelData $(SRC)/Model $(SRC)/Equations ref
O_SER = $(addprefix _ref/obj/ser/,$(addsuffix .o,$(NAMES)))
O_OMP = $(addprefix _ref/obj/omp/,$(addsuffix .o,$(NAMES)))
O_PIC = $(addprefix _ref/obj/pic/,$(addsuffix .o,$(NAMES)))
HDRS = $(wildcard $(SRC)/*/*.hpp) ref/nvector/nvector_serial.h ref/nvector/nvector_openmp.h

all: _ref/shud_ref_f _ref/shud_ref_f_omp _ref/libshud_ref_kat.so
# Our own units are rebuilt when their text changes, whatever the time stamps say: a checkout can leave a changed
# source older than objects built from its earlier version, and a driver without the newer modes would run (and
# exit 0) all the same.  The stamp holds a checksum of our sources and is rewritten only when it differs.
OURS = ref/shud_ref_driver.cpp ref/shud_ref_kat.cpp ref/ref.mk ref/nvector/nvector_serial.h ref/nvector/nvector_openmp.h
_ref/ours.stamp: FORCE
	@mkdir -p _ref
	@cat $(OURS) | cksum > $@.new; if cmp -s $@.new $@; then rm -f $@.new; else mv $@.new $@; fi
FORCE:
_ref/obj/ser/shud_ref_driver.o _ref/obj/omp/shud_ref_driver.o _ref/obj/pic/shud_ref_kat.o: _ref/ours.stamp
_ref/obj/ser/%.o: %.cpp $(HDRS)
	@mkdir -p $(@D)
	$(CXX) $(REFFLAGS) $(INC) -c -o $@ $<
_ref/obj/omp/%.o: %.cpp $(HDRS)
	@mkdir -p $(@D)
	$(CXX) $(REFFLAGS) -D_OPENMP_ON -fopenmp $(INC) -c -o $@ $<
_ref/obj/pic/%.o: %.cpp $(HDRS)
	@mkdir -p $(@D)
	$(CXX) $(REFFLAGS) -fPIC $(INC) -c -o $@ $<
_ref/shud_ref_f: _ref/obj/ser/shud_ref_driver.o $(O_SER)
	$(CXX) -o $@ $^ -lm
_ref/shud_ref_f_omp: _ref/obj/omp/shud_ref_driver.o $(O_OMP)
	$(CXX) -fopenmp -o $@ $^ -lm
_ref/libshud_ref_kat.so: _ref/obj/pic/shud_ref_kat.o $(O_PIC)
	$(CXX) -shared -o $@ $^ -lm
.PHONY: all FORCE
