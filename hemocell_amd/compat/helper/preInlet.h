#pragma once
#include "../preInlet.h"
