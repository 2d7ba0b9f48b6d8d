#pragma once
#include "../bindingField.h"
